"""Records tests/golden/launch_records.json: the ops.PROFILE records (kernel name, algorithmic FLOPs, shape, executed FLOPs) of
the launches in tests/launch_record_cases.py, which tests/test_gpu_launch_records.py compares against.  Needs the GPU.
    python scripts/record_launch_records.py [TREE] [--out FILE]
TREE: another checkout (built) whose simplerecon_amd package -- its ops.py and its library -- makes the launches instead of this
one: the fixture pins the records of the commit BEFORE a change to how they are produced, so it is recorded from that commit
with this tree's cases."""
import fnmatch
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
out = os.path.join(ROOT, "tests", "golden", "launch_records.json")
if "--out" in args:
    out = args.pop(args.index("--out") + 1)
    args.remove("--out")
sys.path[:0] = [os.path.abspath(args[0]) if args else ROOT, os.path.join(ROOT, "tests")]
import launch_record_cases as cases
import simplerecon_amd

records = {cid: cases.run(cid) for cid in cases.CASE_IDS}
names = {r[0] for recs in records.values() for r in recs}
with open(out, "w") as f:
    f.write('{"cus": %d, "records": {\n' % cases.device_cus())   # (a case per line)
    f.write(",\n".join(f" {json.dumps(cid)}: {json.dumps(recs)}" for cid, recs in sorted(records.items())) + "\n}}\n")
missing = [p for p in cases.COVERED if not fnmatch.filter(names, p)]
assert not missing, f"no recorded kernel name matches {missing}; recorded: {sorted(names)}"
assert all(records.values()), [cid for cid, recs in records.items() if not recs]
print(f"{len(records)} cases, {len(names)} kernel names of {os.path.dirname(simplerecon_amd.__file__)} -> {out}")
