"""Metadata-MLP sweep at the hero_cfg3 shape (batch 8, 7 views, 64 planes, 120x160) under two sets of poses:

  bench    synthetic.cost_volume_inputs, what bench.py runs: many (wave, plane, view) triples have no tap in the image
  overlap  all seven views near identity: no wave is dead at any plane (the guard: such scenes must not pay for the skip)

Prints, per set, the dead fraction (numpy, the projection of csrc/sr_common.h) for the 64 pixels per wave the library
chose (sr_mlp_volume_tile_shape under the current SR_MLP_TILE) and for the flattened strip, and the time of
FeatureVolumeManager.forward (HIP events, median of --iters launches).  A/B against another build of the library:
SR_HIP_LIBRARY=/path/to/libsimplerecon_hip.so python scripts/mlp_dead_views_micro.py

Without a GPU:  python scripts/mlp_dead_views_micro.py --cpu [--shape B K D h w] [--seed S]  prints the dead fraction of
synthetic.cost_volume_inputs at that shape for every way of forming a wave (needs the built library only for the shape
the chooser takes).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from simplerecon_amd import synthetic
from simplerecon_amd.cost_volume import FeatureVolumeManager, mlp_tile_shape, mlp_wave_pixels

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


def pixel_taps(inp, planes_bd):
    """tap[b, k, plane, pixel]: the pixel has a tap of view k inside the source image at that plane."""
    n = {k: v.numpy().astype(np.float64) for k, v in inp.items()}
    nb, nk, _, h, w = n["src_feats"].shape
    N = h * w
    ys, xs = np.divmod(np.arange(N), w)
    pix = np.stack([xs + 0.5, ys + 0.5, np.ones(N)])
    tap = np.zeros((nb, nk, planes_bd.shape[1], N), dtype=bool)
    for b in range(nb):
        rays = n["cur_invK"][b, :3, :3] @ pix
        for k in range(nk):
            P = (n["src_Ks"][b, k] @ n["src_extrinsics"][b, k])[:3]
            X = planes_bd[b][:, None, None] * rays[None]                     # [D, 3, N]
            q = np.einsum("ij,djn->din", P[:, :3], X) + P[None, :, 3:4]
            zp = q[:, 2] + 1e-8
            sc = np.where(np.abs(q[:, 2]) > 1e-8, 1.0 / zp, 1.0)
            ix, iy = q[:, 0] * sc - 0.5, q[:, 1] * sc - 0.5
            tap[b, k] = (ix >= -1.0) & (ix < w) & (iy >= -1.0) & (iy < h)
    return tap


def dead_fraction(tap, lanes):
    """Fraction of (wave, plane, view) triples none of whose pixels has a tap; `lanes` [waves, n] holds the flattened pixel
    index of every lane of a wave, -1 for lanes past the image (cost_volume.mlp_wave_pixels)."""
    live = np.concatenate([tap, np.zeros(tap.shape[:-1] + (1,), dtype=bool)], -1)[..., lanes].any(-1)   # -1 -> the False
    return 1.0 - float(live.mean())


def dead_fractions(inp, planes_bd, h, w):
    """The library's choice for this map and the flattened strip."""
    tap = pixel_taps(inp, planes_bd)
    th, tw = mlp_tile_shape(h, w)
    return {"tile": "flat" if th == 1 else f"{th}x{tw}", "dead_fraction": round(dead_fraction(tap, mlp_wave_pixels(h, w)), 4),
            "dead_fraction_flat": round(dead_fraction(tap, mlp_wave_pixels(h, w, (1, 64))), 4)}


def cpu_table(b, k, d, h, w, seed):
    """The dead fraction of the benchmark's poses for every way of forming a wave; no GPU."""
    from simplerecon_amd.cost_volume import CostVolumeManager
    inp = synthetic.cost_volume_inputs(b, k, C, h, w, seed=seed)
    planes = CostVolumeManager(h, w, num_depth_bins=d).generate_depth_planes(b, inp["min_depth"], inp["max_depth"])
    tap = pixel_taps(inp, planes[:, :, 0, 0].numpy().astype(np.float64))
    N = h * w
    rows = [("64 flattened", mlp_wave_pixels(h, w, (1, 64)))]
    strip32 = np.arange(-(-N // 32) * 32).reshape(-1, 32)
    rows.append(("32 flattened", np.where(strip32 < N, strip32, -1)))
    rows += [(f"{th}x{64 // th}", mlp_wave_pixels(h, w, (th, 64 // th))) for th in (2, 4, 8)]
    half = mlp_wave_pixels(h, w, (8, 8)).reshape(-1, 2, 32)          # the two 32-lane halves of an 8x8 tile: 4 rows each
    rows += [("8x8 halves (4x8)", half.reshape(-1, 32)), ("1 pixel", np.arange(N).reshape(-1, 1))]
    th, tw = mlp_tile_shape(h, w)
    chosen = "64 flattened" if th == 1 else f"{th}x{tw}"
    flat_units = len(rows[0][1])
    print(f"B {b}, K {k}, D {d}, {h}x{w}, seed {seed}: dead (wave, plane, view) triples")
    for name, lanes in rows:
        units = f", {100.0 * (len(lanes) / flat_units - 1.0):+.1f} % units" if lanes.shape[1] == 64 and len(lanes) != flat_units else ""
        print(f"  {name:18s} {dead_fraction(tap, lanes):.3f}{units}{'   <- chosen' if name == chosen else ''}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--cpu", action="store_true", help="only the dead-fraction table of --shape / --seed; no GPU")
    ap.add_argument("--shape", type=int, nargs=5, metavar=("B", "K", "D", "h", "w"), default=(B, K, D, H, W))
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    if args.cpu:
        return cpu_table(*args.shape, args.seed)
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
        out[name] = {**dead_fractions(inp, planes, H, W), "ms_median": round(float(np.median(ms)), 4),
                     "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
