"""Times render.vertex_normals and render.render_color next to render.render_depth on the same input: a marching-cubes
mesh of a synthetic TSDF (a sphere, about half a million faces) seen from 8 cameras at 480 x 640.  render_color
rasterises and then shades, so shading alone is render_color minus render_depth; the figure of interest is that
difference relative to render_depth.  Device events around each repeat, warm-up first, median of the repeats
(scripts/bench_frames.py's bracket); a call includes the rasteriser's host synchronisations.

    python scripts/shade_micro.py [--repeats 30] [--warmup 5] [--out profiles/shade_micro.json]

There is no CPU path: without a GPU this script fails."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_frames import gpu_ms  # noqa: E402
from simplerecon_amd import render  # noqa: E402
from simplerecon_amd.tsdf import TriangleMesh, marching_cubes  # noqa: E402

B, H, W = 8, 480, 640


def sphere_mesh(dev, n=240, radius=115.0, vox=0.02):
    ax = torch.arange(n, device=dev, dtype=torch.float32) - (n - 1) / 2.0
    d = torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) - radius
    o = -(n - 1) / 2.0 * vox
    return marching_cubes(d.clamp_(-1.0, 1.0).half(), origin=(o, o, o), scale=vox, compute_normals=False)


def cameras(dev, dist=6.0, focal=500.0):
    """B cameras on a ring around the origin, looking at it."""
    K = torch.eye(4, device=dev).repeat(B, 1, 1)
    K[:, 0, 0] = K[:, 1, 1] = focal
    K[:, 0, 2], K[:, 1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    T = np.zeros((B, 4, 4))
    for b in range(B):
        a = 2 * np.pi * b / B + 0.1
        fwd = -np.array([np.cos(a) * np.cos(0.2), np.sin(0.2), np.sin(a) * np.cos(0.2)])
        down = np.array([0.0, 1.0, 0.0]) - fwd[1] * fwd
        down /= np.linalg.norm(down)
        world_T_cam = np.eye(4)
        world_T_cam[:3, :3], world_T_cam[:3, 3] = np.stack([np.cross(down, fwd), down, fwd], 1), -dist * fwd
        T[b] = np.linalg.inv(world_T_cam)
    return K, torch.from_numpy(T).float().to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shade_micro.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 repeats")
    dev = torch.device("cuda", 0)
    mesh = sphere_mesh(dev)
    V = int(mesh.vertices.shape[0])
    colors = torch.rand((V, 3), generator=torch.Generator().manual_seed(0)).to(dev)
    K, T = cameras(dev)
    lit = TriangleMesh(mesh.vertices, mesh.faces, render.vertex_normals(mesh), colors)
    lights = [render.headlight(intensity=0.6), render.directional_light((0.3, 0.5, 0.8), intensity=0.3),
              render.point_light((0.0, -8.0, 0.0), intensity=20.0)]
    cases = (("render_depth", lambda: render.render_depth(mesh, K, T, H, W)),
             ("vertex_normals", lambda: render.vertex_normals(mesh)),
             ("render_color_lambert_f32", lambda: render.render_color(lit, K, T, H, W, lights=lights)),
             ("render_color_lambert_u8", lambda: render.render_color(lit, K, T, H, W, lights=lights, output="u8")),
             ("render_color_unlit_f32", lambda: render.render_color(lit, K, T, H, W, shading="unlit")),
             ("render_color_lambert_25_lights", lambda: render.render_color(lit, K, T, H, W,
                                                                           lights=render.light_array((0.0, 0.0, 0.0)))),
             ("render_depth_again", lambda: render.render_depth(mesh, K, T, H, W)))
    depth = render.render_depth(mesh, K, T, H, W)
    result = {"device": torch.cuda.get_device_name(0), "views": B, "height": H, "width": W, "vertices": V,
              "faces": int(mesh.faces.shape[0]), "hit_share": float((depth > 0).float().mean()), "repeats": a.repeats,
              "warmup": a.warmup}
    for name, fn in cases:
        med, lo, hi = gpu_ms(fn, a.warmup, a.repeats)
        result[name] = {"ms_median": med, "ms_min": lo, "ms_max": hi}
    raster = result["render_depth"]["ms_median"]
    for name in ("render_color_lambert_f32", "render_color_lambert_u8", "render_color_unlit_f32",
                 "render_color_lambert_25_lights"):
        result[name]["shading_over_raster"] = (result[name]["ms_median"] - raster) / raster
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
