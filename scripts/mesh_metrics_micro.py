"""Times the mesh metrics (simplerecon_amd.mesh_metrics) at room scale: the ground truth is synthetic.raycast_scene_mesh
at 1 cm spacing, the prediction the same mesh displaced by up to 1.7 cm with the walls beyond x = 2 m cut away (so
completeness queries there are far from any predicted point and walk the coarse grid).

    python scripts/mesh_metrics_micro.py [--iters 5]      # device-event times per call, JSON line
    rocprofv3 --kernel-trace --stats -d DIR -o run -- python scripts/mesh_metrics_micro.py --hip-only --iters 3

Reported: both protocols end to end (vertices with and without the 2 cm downsampling, surface with 1M samples per
mesh), the two nearest-neighbour passes on about 1M x 1M points, the far queries (the completeness queries farther
than two fine cells from the prediction) timed on their own, a chunked fp32 torch brute force on the GPU extrapolated
from a slice of the queries, and scipy's cKDTree(workers=16) when scipy imports."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
from simplerecon_amd import mesh_metrics as mm  # noqa: E402
from simplerecon_amd import synthetic  # noqa: E402
from simplerecon_amd.tsdf import TriangleMesh  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def scenes(dev):
    gt = synthetic.raycast_scene_mesh(0, spacing=0.01)
    v = gt.vertices + 0.01 * torch.sin(gt.vertices * 7.0)
    keep = v[:, 0] < 2.0
    remap = torch.cumsum(keep.long(), 0) - 1
    f = gt.faces.long()
    fk = keep[f].all(1)
    pred = TriangleMesh(v[keep].contiguous(), remap[f[fk]].int().contiguous())
    return (TriangleMesh(gt.vertices.to(dev), gt.faces.to(dev)),
            TriangleMesh(pred.vertices.to(dev), pred.faces.to(dev)))


def brute_ms(q, p, chunk=512):
    def run():
        for s in range(0, len(q), chunk):
            qq = q[s:s + chunk]
            dx = qq[:, None, 0] - p[None, :, 0]
            dy = qq[:, None, 1] - p[None, :, 1]
            dz = qq[:, None, 2] - p[None, :, 2]
            (dx * dx + dy * dy + dz * dz).min(1)
    return timed(run, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--hip-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda")
    gt, pred = scenes(dev)
    res = {"gt_vertices": int(gt.vertices.shape[0]), "pred_vertices": int(pred.vertices.shape[0]), "iters": a.iters}
    runs = {
        "vertices_ds2cm_ms": lambda: mm.mesh_metrics(pred, gt),
        "vertices_full_ms": lambda: mm.mesh_metrics(pred, gt, down_sample=None),
        "surface_1M_ms": lambda: mm.mesh_metrics(pred, gt, sampling="surface", n_points=1_000_000),
    }
    for k, fn in runs.items():
        res[k] = timed(fn, a.iters)
    res["metrics_surface_1M"] = mm.mesh_metrics(pred, gt, sampling="surface", n_points=1_000_000)
    if a.hip_only:
        print(json.dumps(res))
        return
    P = mm.sample_surface(pred, 1_000_000, seed=0).points
    G = mm.sample_surface(gt, 1_000_000, seed=0).points
    res["nn_pred_to_gt_ms"] = timed(lambda: mm.nearest_distances(P, G), a.iters)
    res["nn_gt_to_pred_ms"] = timed(lambda: mm.nearest_distances(G, P), a.iters)
    box = mm._boxes(P)[0]
    grid = mm._TargetGrid(P, box)
    res["pred_grid"] = {"cell_m": grid.cell, "dims": grid.dims, "table_entries": grid.entries}
    res["grid_build_ms"] = timed(lambda: mm._TargetGrid(P, box), a.iters)
    d = grid.query(G)[1]
    far = d > 2 * grid.cell
    Gf, Gn = G[far].contiguous(), G[~far].contiguous()
    res["far_queries"] = int(far.sum())
    res["far_query_ms"] = timed(lambda: grid.query(Gf), a.iters)
    res["near_query_ms"] = timed(lambda: grid.query(Gn), a.iters)
    sl = 8192
    res["brute_slice_queries"] = sl
    res["brute_pred_to_gt_ms_est"] = brute_ms(P[:sl], G) * len(P) / sl
    try:
        import numpy as np
        from scipy.spatial import cKDTree
        p_np, g_np = P.cpu().numpy().astype(np.float64), G.cpu().numpy().astype(np.float64)
        t0 = time.perf_counter()
        tree = cKDTree(g_np)
        tree.query(p_np, workers=16)
        res["ckdtree_pred_to_gt_ms"] = (time.perf_counter() - t0) * 1e3
    except ImportError as e:
        res["ckdtree_pred_to_gt_ms"] = f"not measured: {e}"
    print(json.dumps(res))


if __name__ == "__main__":
    main()
