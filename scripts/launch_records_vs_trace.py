"""Do the ops.PROFILE records name the kernels that ran?  Runs the cases of tests/launch_record_cases.py in a fresh child
process under `rocprofv3 --kernel-trace --stats` (a run of its own, no counters, under a time limit) and compares, in launch
order, each record with the main kernel the profiler traced:
  * the base name must be equal;
  * the record's template-argument list must equal the LEADING template arguments of the traced instantiation (the trace also
    shows defaulted trailing ones, such as the I/O format);
  * sr_pw_tiled_kernel is recorded by its workgroup tile and K split, `<64x128, ks 2, false>`, not by its template arguments
    <WM, WN, NTW, GATE>: the tile must be 32 WM x 32 WN NTW (csrc/sr_pw_tiled.hip, pt_launch), the K split the grid's y size.
    python scripts/launch_records_vs_trace.py OUT_DIR      # writes OUT_DIR/launch_records_vs_trace.txt; exit 1 on a mismatch
An OUT_DIR that already holds a run (records.json and the trace) is only compared again, which needs no GPU."""
import csv
import glob
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAIN = {"sr_conv_kernel", "sr_wino_kernel", "sr_wino_split_kernel", "sr_wino4_kernel", "sr_wino4pp_kernel", "sr_wino4ws_kernel",
        "sr_pw_kernel", "sr_pw_tiled_kernel", "sr_stem_kernel", "sr_conv1x1_stats_kernel", "sr_t16_kernel"}


def child(out):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import launch_record_cases as cases
    records = [(cid, r[0]) for cid in cases.CASE_IDS for r in cases.run(cid)]
    with open(out, "w") as f:
        json.dump(records, f)


def split_name(name):
    """'void k<a, b>(P)' or 'k<a, b>' -> ('k', ['a', 'b'])"""
    m = re.match(r"(?:void )?(\w+)(?:<([^<>]*)>)?(?:\(.*)?$", name.strip().replace("(anonymous namespace)::", ""))
    if m is None:   # (named namespaces, nested templates: none of this library's kernels)
        return name, []
    return m.group(1), ([a.strip() for a in m.group(2).split(",")] if m.group(2) else [])


def matches(record, row):
    base, args = split_name(record)
    tbase, targs = split_name(row["Kernel_Name"])
    if base != tbase:
        return False
    if base == "sr_pw_tiled_kernel":
        wm, wn, ntw = (int(a) for a in targs[:3])
        ksplit = int(row["Grid_Size_Y"]) // int(row["Workgroup_Size_Y"])
        return args == [f"{32 * wm}x{32 * wn * ntw}", f"ks {ksplit}", targs[3]]
    return args == targs[:len(args)]


def main(out_dir):
    os.makedirs(out_dir, exist_ok=True)
    rec_path = os.path.join(out_dir, "records.json")
    if not os.path.exists(rec_path):   # (an OUT_DIR that holds a run is compared again without a GPU)
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", os.path.join(out_dir, "trace"),
                        "-o", "run", "--", sys.executable, os.path.abspath(__file__), "--child", rec_path], check=True, timeout=300)
    with open(rec_path) as f:
        records = json.load(f)
    trace, = glob.glob(os.path.join(out_dir, "trace", "**", "*kernel_trace.csv"), recursive=True)
    with open(trace) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    rows = [r for r in rows if split_name(r["Kernel_Name"])[0] in MAIN]
    lines = [f"{len(records)} records against the {len(rows)} main-kernel launches of the trace, in launch order", "",
             f"{'case':22s} {'ok':3s} {'record':42s} traced"]
    bad = len(records) != len(rows)
    for (cid, name), row in zip(records, rows):
        ok = matches(name, row)
        bad |= not ok
        traced = row["Kernel_Name"].replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0]
        if split_name(name)[0] == "sr_pw_tiled_kernel":
            traced += f"  grid y {row['Grid_Size_Y']} / {row['Workgroup_Size_Y']}"
        lines.append(f"{cid:22s} {'yes' if ok else 'NO':3s} {name:42s} {traced}")
    lines += ["", "MISMATCH" if bad else "every record names the kernel that ran"]
    text = "\n".join(lines) + "\n"
    with open(os.path.join(out_dir, "launch_records_vs_trace.txt"), "w") as f:
        f.write(text)
    print(text)
    return 1 if bad else 0


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2])
    else:
        sys.exit(main(sys.argv[1]))
