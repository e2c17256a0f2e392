"""Point-cloud fusion timing on ray-cast scenes at 480 x 640: python scripts/pc_fusion_micro.py [--frames 32 128 512]

For each N: fuse_scene (consistency kernel + compaction) and voxel_down_sample(0.02) of its result, timed with device
events after warm-up (median of the repeats); pairs/s = N (N - 1) h w / fusion time.  The VALU-issue floor comes from
the consistency kernel's loop body in the ISA (hipcc --save-temps): VALU instructions per iteration (kUnroll sources)
x 2 cycles per wave64 instruction on a SIMD-32 x iterations x waves, over 1024 SIMDs at 2.4 GHz.  The batched-torch
restatement of the rules (tests/pc_oracle.torch_fuse, 100 sources per batch as the reference batches them) is timed on
the same GPU for N <= --torch-max-frames."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
from simplerecon_amd import build, point_cloud, synthetic  # noqa: E402

DEV = "cuda:0"
H, W = 480, 640
UNROLL = 4          # kUnroll of csrc/sr_pcfusion.hip
SIMDS, CLOCK = 1024, 2.4e9


def loop_valu():
    """(VALU instructions, of which packed) in the consistency kernel's source loop."""
    src = os.path.join(build.CSRC, "sr_pcfusion.hip")
    with tempfile.TemporaryDirectory() as td:
        cmd = [build.HIPCC] + build.FLAGS + ["--save-temps", "-c", src, "-o", os.path.join(td, "pc.o")]
        subprocess.run(cmd, cwd=td, check=True, capture_output=True)
        asm = open(next(os.path.join(td, f) for f in os.listdir(td) if f.endswith("gfx950.s"))).read()
    body = asm[asm.index("sr_pc_consistency_kernel"):]
    body = body[:body.index("s_endpgm")]
    # the loop: from the label that a backward s_cbranch jumps to, up to that branch
    for m in re.finditer(r"s_cbranch_\w+ (\.LBB\d+_\d+)", body):
        lab = m.group(1)
        start = body.find(lab + ":")
        if 0 <= start < m.start():
            insts = [ln.split()[0] for ln in body[start:m.start()].splitlines()[1:] if ln.strip() and
                     not ln.strip().startswith((";", "."))]
            valu = [i for i in insts if i.startswith("v_")]
            return len(valu), sum(i.startswith("v_pk_") for i in valu)
    raise RuntimeError("loop not found in the ISA")


def timed(fn, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    out, ts = None, []
    for _ in range(reps):
        ev[0].record()
        out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        ts.append(ev[0].elapsed_time(ev[1]))
    ts.sort()
    return ts[len(ts) // 2], out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[32, 128, 512])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-max-frames", type=int, default=128)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pc_fusion_micro needs a GPU"
    import pc_oracle
    valu, packed = loop_valu()
    print(json.dumps({"loop_valu_per_iteration": valu, "packed": packed, "sources_per_iteration": UNROLL}), flush=True)
    for N in a.frames:
        sc = synthetic.raycast_scene(N, H, W, seed=N, noise=0.002, holes=0.01, device=DEV)
        args = (sc["depths"], sc["images"], sc["cam_T_world"], sc["K"])
        point_cloud.fuse_scene(*args)                                   # warm-up
        t_fuse, (pc, valid) = timed(lambda: point_cloud.fuse_scene(*args), a.reps)
        point_cloud.PointCloud(pc.points, pc.colors).voxel_down_sample(0.02)
        t_vox, down = timed(lambda: pc.voxel_down_sample(0.02), a.reps)
        pairs = N * (N - 1) * H * W
        waves = N * ((H * W + 63) // 64)
        floor_s = waves * -(-N // UNROLL) * valu * 2 / (SIMDS * CLOCK)
        rec = {"N": N, "fuse_ms": round(t_fuse, 3), "pairs_per_s": pairs / (t_fuse * 1e-3),
               "valu_floor_ms": round(floor_s * 1e3, 3), "fraction_of_floor": round(floor_s * 1e3 / t_fuse, 3),
               "kept_points": len(pc), "kept_fraction": round(float(valid.float().mean()), 4),
               "voxel_ms": round(t_vox, 3), "voxels": len(down)}
        if N <= a.torch_max_frames:
            zt = 0.04
            t_torch, _ = timed(lambda: pc_oracle.torch_fuse(sc["depths"], sc["cam_T_world"], sc["K"], zt, 3), 2)
            rec.update(torch_ms=round(t_torch, 3), speedup_vs_torch=round(t_torch / t_fuse, 1))
        print(json.dumps(rec), flush=True)
        del sc, args, pc, valid, down
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
