"""Per-kernel code-object metadata of .hip translation units, for comparing two trees without a GPU.

    python scripts/codeobj_meta.py [--root TREE] sr_mesh.hip sr_losses.hip ... > table.txt

Compiles the device side of each file with the flags of simplerecon_amd/build.py and prints, per kernel, the VGPR and
SGPR counts, LDS and scratch bytes (the AMDGPU metadata note), the code size (the kernel symbol's size) and a digest of
the symbol's bytes in .text.  Two trees whose tables are equal run the same machine code per kernel, not merely the same
register/LDS budget."""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
FIELDS = (("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("lds", ".group_segment_fixed_size"),
          ("scratch", ".private_segment_fixed_size"))


def kernels(root, name, tmp):
    sys.path.insert(0, root)
    from simplerecon_amd import build as b
    co = os.path.join(tmp, name + ".co")
    subprocess.run([b.HIPCC] + b.FLAGS + ["--cuda-device-only", "--no-gpu-bundle-output", "-c", os.path.join(b.CSRC, name),
                                          "-o", co], check=True, capture_output=True)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", co], check=True, capture_output=True, text=True).stdout
    sym_re = r"^\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+FUNC\s.*\s(\S+)$"
    addr = {m.group(3): (int(m.group(1), 16), int(m.group(2))) for m in re.finditer(sym_re, syms, re.M)}
    secs = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-SW", co], check=True, capture_output=True, text=True).stdout
    text_addr, text_off = (int(x, 16) for x in re.search(r"\s\.text\s+PROGBITS\s+([0-9a-f]+)\s+([0-9a-f]+)", secs).groups())
    with open(co, "rb") as fh:
        image = fh.read()
    out = {}
    for block in notes.split("  - .agpr_count:")[1:]:
        rec = {key: int(re.search(re.escape(field) + r":\s+(\d+)", block).group(1)) for key, field in FIELDS}
        sym = re.search(r"\.name:\s+(\S+)", block).group(1)
        start, rec["code"] = addr[sym]
        start += text_off - text_addr
        rec["digest"] = hashlib.sha256(image[start:start + rec["code"]]).hexdigest()[:16]
        out[sym] = rec
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("files", nargs="+")
    a = ap.parse_args()
    print(f"{'file':22s} {'vgpr':>5s} {'sgpr':>5s} {'lds':>6s} {'scratch':>7s} {'code':>6s} {'digest':16s}  kernel")
    with tempfile.TemporaryDirectory() as tmp:
        for f in a.files:
            for sym, r in sorted(kernels(os.path.abspath(a.root), f, tmp).items()):
                print(f"{f:22s} {r['vgpr']:5d} {r['sgpr']:5d} {r['lds']:6d} {r['scratch']:7d} {r['code']:6d} {r['digest']}  {sym}")


if __name__ == "__main__":
    main()
