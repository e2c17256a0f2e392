"""Times the fused test-time scoring (metrics.score_frames: nearest gather + batched rule, two launches) against a
fresh fp32 ATen restatement of the same work as test.py does it (F.interpolate(mode="nearest"), then the batched rule
with NaN fill, stacked ratios, seven masks and nanmeans), on the same device, at B=8, pred 192x256 -> gt 480x640.

    python scripts/metrics_micro.py [--iters 200]                 # wall time per call, device events
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/metrics_micro.py --hip-only --iters 200
    python scripts/metrics_micro.py --hip-only --iters 5 --stats DIR/.../run_results.db

The second form traces the kernels; the third reads the trace database rocprofv3 writes and prints the mean time of
each metrics kernel and the bytes the tile pass moves over its time, against the HBM peak (8 TB/s)."""
import argparse
import json
import os
import re
import sqlite3
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from simplerecon_amd import metrics, synthetic  # noqa: E402

HBM_PEAK = 8.0e12


def aten_score(gt_b1HW, pred_b1hw, min_depth=0.5):
    """test.py:263-277 + compute_depth_metrics_batched, restated in fp32 ATen."""
    up = F.interpolate(pred_b1hw, size=gt_b1HW.shape[-2:], mode="nearest")
    valid = (gt_b1HW > min_depth).flatten(1)
    gt = gt_b1HW.flatten(1).clone()
    pred = up.flatten(1).clone()
    gt[~valid] = torch.nan
    pred[~valid] = torch.nan
    thresh = torch.max(torch.stack([gt / pred, pred / gt], dim=2), dim=2)[0]
    out = {}
    for k, t in (("a5", 1.05), ("a10", 1.1), ("a25", 1.25), ("a0", 1.1), ("a1", 1.25), ("a2", 1.25 ** 2),
                 ("a3", 1.25 ** 3)):
        a = (thresh < t).float()
        a[~valid] = torch.nan
        out[k] = torch.nanmean(a, dim=1) * 100
    d = gt - pred
    out["rmse"] = torch.sqrt(torch.nanmean(d ** 2, dim=1))
    out["rmse_log"] = torch.sqrt(torch.nanmean((torch.log(gt) - torch.log(pred)) ** 2, dim=1))
    out["abs_rel"] = torch.nanmean(torch.abs(d) / gt, dim=1)
    out["sq_rel"] = torch.nanmean(d ** 2 / gt, dim=1)
    out["abs_diff"] = torch.nanmean(torch.abs(d), dim=1)
    return out


def timed(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--hip-only", action="store_true")
    ap.add_argument("--stats", help="results database of a rocprofv3 --kernel-trace run of --hip-only")
    a = ap.parse_args()
    B, H, W, h, w = 8, 480, 640, 192, 256
    gt = synthetic.raycast_scene(B, H, W, seed=3, holes=0.02)["depths"].float().unsqueeze(1).cuda()
    pred = synthetic.raycast_scene(B, h, w, seed=3, noise=0.05)["depths"].float().unsqueeze(1).cuda()
    # bytes the fused pass must move: gt once, the prediction once (it stays in cache across its reuse)
    nbytes = gt.numel() * 4 + pred.numel() * 4
    res = {"B": B, "gt": [H, W], "pred": [h, w], "bytes": nbytes, "iters": a.iters}
    res["hip_ms"] = timed(lambda: metrics.score_frames(gt, pred), a.iters)
    if not a.hip_only:
        res["aten_ms"] = timed(lambda: aten_score(gt, pred), a.iters)
        res["speedup"] = res["aten_ms"] / res["hip_ms"]
        for label, fn in (("hip_kernels", lambda: metrics.score_frames(gt, pred)),
                          ("aten_kernels", lambda: aten_score(gt, pred))):
            try:
                with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
                    fn()
                    torch.cuda.synchronize()
                res[label] = sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)
            except Exception as e:   # the count is informative only; the times above stand without it
                res[label] = f"not counted: {e}"
        # agreement of the two on this data
        m, _ = metrics.score_frames(gt, pred)
        ref = aten_score(gt, pred)
        res["max_rel_diff"] = max(float(((m[k] - ref[k]).abs() / ref[k].abs()).max()) for k in metrics.METRIC_KEYS)
    if a.stats:
        db = sqlite3.connect(a.stats)
        q = "select name, avg(end - start) from kernels where name like '%sr_metrics%' group by name"
        kern = {re.search(r"(sr_metrics_\w+)", name).group(1): ns * 1e-3 for name, ns in db.execute(q)}
        res["kernel_us"] = kern
        tile = sum(v for k, v in kern.items() if "tile" in k)
        if tile:
            res["tile_pass_GBps"] = nbytes / (tile * 1e-6) / 1e9
            res["tile_pass_frac_of_hbm_peak"] = nbytes / (tile * 1e-6) / HBM_PEAK
    print(json.dumps(res))


if __name__ == "__main__":
    main()
