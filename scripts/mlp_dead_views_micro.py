"""Metadata-MLP sweep at the hero_cfg3 shape (batch 8, 7 views, 64 planes, 120x160) under two sets of poses:

  bench    synthetic.cost_volume_inputs, what bench.py runs: many (wave, plane, view) triples have no tap in the image
  overlap  all seven views near identity: no wave is dead at any plane (the guard: such scenes must not pay for the skip)

Prints, per set, the dead fraction (numpy, the projection of csrc/sr_common.h, 64-pixel waves in flattened pixel order) and
the time of FeatureVolumeManager.forward (HIP events, median of --iters launches).  A/B against another build of the
library: SR_HIP_LIBRARY=/path/to/libsimplerecon_hip.so python scripts/mlp_dead_views_micro.py
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from simplerecon_amd import synthetic
from simplerecon_amd.cost_volume import FeatureVolumeManager

B, K, C, D, H, W = 8, 7, 16, 64, 120, 160


def overlap_inputs(seed=0):
    """The benchmark's inputs with every source camera within 2 mm of the reference camera."""
    inp = synthetic.cost_volume_inputs(B, K, C, H, W, seed=seed)
    rng = np.random.default_rng(77)
    extr = np.tile(np.eye(4), (B, K, 1, 1))
    extr[:, :, :3, 3] = rng.uniform(-0.002, 0.002, size=(B, K, 3))
    inp["src_extrinsics"] = torch.from_numpy(extr.astype(np.float32))
    inp["src_poses"] = torch.from_numpy(np.linalg.inv(extr).astype(np.float32))
    return inp


def dead_fraction(inp, planes_bd):
    """Fraction of (wave, plane, view) triples none of whose pixels has a tap inside the source image."""
    n = {k: v.numpy().astype(np.float64) for k, v in inp.items()}
    N = H * W
    ys, xs = np.divmod(np.arange(N), W)
    pix = np.stack([xs + 0.5, ys + 0.5, np.ones(N)])
    pad = (-N) % 64
    dead = total = 0
    for b in range(B):
        rays = n["cur_invK"][b, :3, :3] @ pix
        for k in range(K):
            P = (n["src_Ks"][b, k] @ n["src_extrinsics"][b, k])[:3]
            X = planes_bd[b][:, None, None] * rays[None]                     # [D, 3, N]
            q = np.einsum("ij,djn->din", P[:, :3], X) + P[None, :, 3:4]
            zp = q[:, 2] + 1e-8
            sc = np.where(np.abs(q[:, 2]) > 1e-8, 1.0 / zp, 1.0)
            ix, iy = q[:, 0] * sc - 0.5, q[:, 1] * sc - 0.5
            tap = (ix >= -1.0) & (ix < W) & (iy >= -1.0) & (iy < H)
            tap = np.pad(tap, ((0, 0), (0, pad))).reshape(D, -1, 64).any(-1)
            dead += int((~tap).sum())
            total += tap.size
    return dead / total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    mgr = FeatureVolumeManager(H, W, num_depth_bins=D, matching_dim_size=C, num_source_views=K)
    synthetic.seeded_fill_(mgr.mlp, seed=3)
    mgr = mgr.to(dev)
    mgr.volume_memory_format = torch.channels_last
    out = {"library": os.environ.get("SR_HIP_LIBRARY", "in-tree")}
    for name, inp in (("bench", synthetic.cost_volume_inputs(B, K, C, H, W, seed=0)), ("overlap", overlap_inputs())):
        dinp = {k: v.to(dev) for k, v in inp.items()}
        with torch.inference_mode():
            for _ in range(3):
                res = mgr(return_mask=True, **dinp)
            ms = []
            for _ in range(args.iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                res = mgr(return_mask=True, **dinp)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
        planes = res[2][:, :, 0, 0].cpu().numpy().astype(np.float64)
        out[name] = {"dead_fraction": round(dead_fraction(inp, planes), 4), "ms_median": round(float(np.median(ms)), 4),
                     "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
