"""Sparse TSDF micro-benchmark: batch-8 integration of 640x480 depth maps along bench_workloads.TsdfFuse's trajectory
(random depth in [1, 2.5] m, 5 cm steps along x with a slow yaw) into a ScalableTSDFVolume at 4 cm, then mesh extraction,
next to the dense OurFuser (TsdfFuse itself: 504^3 fp16 volume) on the same frames.

Device-event medians per step: integration = touch + unique / mask / merge (with its host synchronisations) and the
integrate kernel; extraction = mesh count, totals readback, emit (vertices + faces).  Events are recorded around the
library calls by wrapping them, so the product code runs unchanged.

    python scripts/scalable_tsdf_micro.py [--steps 30] [--warmup 5] [--out scalable_tsdf_micro.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench_workloads  # noqa: E402
from simplerecon_amd import _lib  # noqa: E402
from simplerecon_amd.scalable_tsdf import ScalableTSDFVolume  # noqa: E402


class _Marks:
    """Wraps library entry points so that a CUDA event is recorded right before and after each call."""

    def __init__(self, lib, names):
        self.ev = {}
        for n in names:
            fn = getattr(lib, n)

            def wrapped(*args, _fn=fn, _n=n):
                a = torch.cuda.Event(enable_timing=True)
                b = torch.cuda.Event(enable_timing=True)
                a.record()
                rc = _fn(*args)
                b.record()
                self.ev[_n] = (a, b)
                return rc
            setattr(lib, n, wrapped)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = _lib.lib()
    marks = _Marks(lib, ["sr_stsdf_integrate", "sr_stsdf_mesh_count", "sr_stsdf_mesh_emit"])
    wl = bench_workloads.TsdfFuse(dev, 0)
    depth32, K32 = wl.depth.float(), wl.K.float()
    vol = ScalableTSDFVolume(0.04, 0.12, 3.0, device=dev)
    res = {"touch_merge_ms": [], "integrate_ms": [], "call_ms": [], "call_wall_ms": [], "dense_ms": [],
           "new_blocks": [], "blocks_total": []}
    for i in range(a.warmup + a.steps):
        T = wl._poses(i + 1).float()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        n0 = vol.num_blocks
        s.record()
        vol.integrate(depth32, K32, T)
        e.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - w0) * 1e3
        i0, i1 = marks.ev["sr_stsdf_integrate"]
        ds, de = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ds.record()
        wl.fuser.tsdf_fuser_pred.integrate_depth(wl.depth, T.half(), wl.K)
        de.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            res["touch_merge_ms"].append(s.elapsed_time(i0))
            res["integrate_ms"].append(i0.elapsed_time(i1))
            res["call_ms"].append(s.elapsed_time(e))
            res["call_wall_ms"].append(wall)
            res["dense_ms"].append(ds.elapsed_time(de))
            res["blocks_total"].append(vol.num_blocks)
            res["new_blocks"].append(vol.num_blocks - n0)
    mesh_t = {"count_ms": [], "readback_ms": [], "emit_ms": [], "total_ms": []}
    for i in range(a.warmup + 10):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        mesh = vol.extract_mesh()
        e.record()
        torch.cuda.synchronize()
        c0, c1 = marks.ev["sr_stsdf_mesh_count"]
        m0, m1 = marks.ev["sr_stsdf_mesh_emit"]
        if i >= a.warmup:
            mesh_t["count_ms"].append(c0.elapsed_time(c1))
            mesh_t["readback_ms"].append(c1.elapsed_time(m0))
            mesh_t["emit_ms"].append(m0.elapsed_time(m1))
            mesh_t["total_ms"].append(s.elapsed_time(e))
    med = lambda x: float(np.median(x))  # noqa: E731
    out = {
        "integration_batch8_640x480": {k: med(v) for k, v in res.items() if k.endswith("_ms")},
        "new_blocks_per_step_median": med(res["new_blocks"]),
        "blocks_after": int(vol.num_blocks),
        "pool_mb": vol.capacity * 5 * 4096 * 4 / 2 ** 20,
        "extraction": {k: med(v) for k, v in mesh_t.items()},
        "mesh": {"vertices": int(mesh.vertices.shape[0]), "faces": int(mesh.faces.shape[0])},
        "steps": a.steps, "warmup": a.warmup,
    }
    print(json.dumps(out, indent=1))
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)


if __name__ == "__main__":
    main()
