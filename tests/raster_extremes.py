"""The two extreme workloads of the rasteriser (and one in between), timed: run as a program by tests/test_gpu_raster.py (each in a child
process under a time limit) and by hand for the figures in DESIGN.md.

    python tests/raster_extremes.py full_frame|midsize|million [repeats]

Prints one JSON line: the case's sizes, ms per render_depth call (device events, two warm-ups, median of `repeats`), ns per
pixel, and the plausibility figures the test asserts on."""
import json
import sys

import numpy as np
import torch

DEV = "cuda:0"


def _time(fn, repeats):
    """Median ms of `repeats` calls between device events, after two warm-up calls.  A call includes render_depth's
    host synchronisations (it cannot size the large-triangle pass without one)."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return out, float(np.median(ms))


def full_frame(repeats):
    """Two triangles covering a 1920 x 1440 frame: a tilted wall."""
    from simplerecon_amd.render import render_depth
    from simplerecon_amd.tsdf import TriangleMesh
    H, W = 1440, 1920
    v = torch.tensor([[-9.0, -7.0, 3.0], [9.0, -7.0, 5.0], [9.0, 7.0, 5.0], [-9.0, 7.0, 3.0]], device=DEV)
    f = torch.tensor([[0, 3, 2], [0, 2, 1]], dtype=torch.int32, device=DEV)
    K = torch.eye(4, device=DEV)[None].clone()
    K[0, 0, 0] = K[0, 1, 1] = 1500.0
    K[0, 0, 2], K[0, 1, 2] = 959.5, 719.5
    T = torch.eye(4, device=DEV)[None]
    depth, ms = _time(lambda: render_depth(TriangleMesh(v, f), K, T, H, W), repeats)
    # the plane through the wall: z = 4 + x / 9, along the ray (rx, ry, 1): z = 4 / (1 - rx / 9)
    rx = (torch.arange(W, device=DEV, dtype=torch.float64) - 959.5) / 1500.0
    want = (4.0 / (1.0 - rx / 9.0)).float()[None, :].expand(H, W)
    err = float(((depth[0, 0] - want).abs() / want).max())
    return dict(case="full_frame", faces=2, views=1, height=H, width=W, ms=ms, ns_per_pixel=ms * 1e6 / (H * W),
                hit_share=float((depth > 0).float().mean()), max_rel_err=err)


def midsize(repeats):
    """9600 triangles whose boxes are just above the small-path limit (24 x 24 pixels each), tiling a 1920 x 1440 frame:
    the worst case for the large path's per-tile setup.  Timing only (plus: every pixel is hit)."""
    from simplerecon_amd.render import render_depth
    from simplerecon_amd.tsdf import TriangleMesh
    H, W, nx, ny = 1440, 1920, 80, 60
    xs = torch.linspace(-0.7, 0.7, nx + 1, device=DEV, dtype=torch.float64) * (W / 1500.0) * 4.0 * (nx / (nx - 2.0)) / 1.4
    ys = torch.linspace(-0.7, 0.7, ny + 1, device=DEV, dtype=torch.float64) * (H / 1500.0) * 4.0 * (ny / (ny - 2.0)) / 1.4
    X, Y = torch.meshgrid(xs, ys, indexing="ij")
    v = torch.stack([X, Y, torch.full_like(X, 4.0)], -1).reshape(-1, 3).float().contiguous()
    i = (torch.arange(nx, device=DEV)[:, None] * (ny + 1) + torch.arange(ny, device=DEV)[None, :]).reshape(-1)
    f = torch.cat([torch.stack([i, i + 1, i + ny + 2], 1), torch.stack([i, i + ny + 2, i + ny + 1], 1)]).int().contiguous()
    K = torch.eye(4, device=DEV)[None].clone()
    K[0, 0, 0] = K[0, 1, 1] = 1500.0
    K[0, 0, 2], K[0, 1, 2] = 959.5, 719.5
    T = torch.eye(4, device=DEV)[None]
    depth, ms = _time(lambda: render_depth(TriangleMesh(v, f), K, T, H, W), repeats)
    return dict(case="midsize", faces=int(f.shape[0]), views=1, height=H, width=W, ms=ms, ns_per_pixel=ms * 1e6 / (H * W),
                hit_share=float((depth > 0).float().mean()), max_abs_err=float((depth - 4.0).abs().max()))


def million(repeats):
    """A marching-cubes sphere of more than a million faces into 8 views of 640 x 480."""
    from simplerecon_amd.render import render_depth
    from simplerecon_amd.tsdf import marching_cubes
    n, R, vox = 480, 230.0, 0.01
    ax = torch.arange(n, device=DEV, dtype=torch.float32) - (n - 1) / 2.0
    d = torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) - R
    vol = d.clamp_(-1.0, 1.0).half()
    del d
    o = -(n - 1) / 2.0 * vox
    mesh = marching_cubes(vol, origin=(o, o, o), scale=vox, compute_normals=False)
    del vol
    H, W, B, dist, focal = 480, 640, 8, 6.0, 500.0
    K = torch.eye(4, device=DEV).repeat(B, 1, 1)
    K[:, 0, 0] = K[:, 1, 1] = focal
    K[:, 0, 2], K[:, 1, 2] = 319.5, 239.5
    T = torch.zeros((B, 4, 4), dtype=torch.float64)
    for b in range(B):
        a = 2 * np.pi * b / B + 0.1
        fwd = -np.array([np.cos(a) * np.cos(0.2), np.sin(0.2), np.sin(a) * np.cos(0.2)])
        down = np.array([0.0, 1.0, 0.0]) - fwd[1] * fwd
        down /= np.linalg.norm(down)
        Rm = np.stack([np.cross(down, fwd), down, fwd], 1)       # world_T_cam rotation
        wTc = np.eye(4)
        wTc[:3, :3], wTc[:3, 3] = Rm, -dist * fwd
        T[b] = torch.from_numpy(np.linalg.inv(wTc))
    T = T.float().to(DEV)
    depth, ms = _time(lambda: render_depth(mesh, K, T, H, W), repeats)
    # analytic sphere of radius R vox about the origin, camera at distance `dist` on its axis
    u = (torch.arange(W, device=DEV, dtype=torch.float64) - 319.5) / focal
    v = (torch.arange(H, device=DEV, dtype=torch.float64) - 239.5) / focal
    r2 = 1.0 + u[None, :] ** 2 + v[:, None] ** 2
    rad = R * vox
    disc = dist * dist - r2 * (dist * dist - rad * rad)
    z = (dist - torch.sqrt(disc.clamp(min=0))) / r2
    cosang = torch.sqrt(disc.clamp(min=0) / r2) / rad               # |n . r| at the hit
    inner = (disc > 0) & (cosang > 0.3)
    outside = disc < -0.02 * dist * dist
    got = depth[:, 0].double()
    err = float((got - z)[:, inner].abs().max())
    return dict(case="million", faces=int(mesh.faces.shape[0]), views=B, height=H, width=W, ms=ms,
                ns_per_pixel=ms * 1e6 / (B * H * W), inner_hit_share=float((got[:, inner] > 0).double().mean()),
                inner_max_abs_err=err, outside_hit_share=float((got[:, outside] > 0).double().mean()), voxel=vox)


if __name__ == "__main__":
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    print(json.dumps({"full_frame": full_frame, "midsize": midsize, "million": million}[sys.argv[1]](reps)))
