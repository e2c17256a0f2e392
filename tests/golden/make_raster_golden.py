"""Writes tests/golden/raster_<scene>.npz: the meshes and cameras the rasteriser is checked on (tests/raster_cases.py
loads them).  Scenes are inputs only; the expected renders come from tests/raster_oracle.py at test time.

    python tests/golden/make_raster_golden.py

Every scene is laid out in the frame of its first camera (x right, y down, z forward) and then moved into a world
frame by a fixed pose, so camera and world axes never coincide.  Stored per scene: vertices [V,3] fp32, faces [F,3]
int32, cam_T_world [5,4,4] fp32 (view 0 is the scene's own camera, the others look at it from nearby), hidden [n] int32
(faces that lie wholly behind the occluder in view 0; empty where the scene has none)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    x, y, z = axis
    Kx = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def _pose(axis, angle, t):
    T = np.eye(4)
    T[:3, :3] = _rot(axis, angle)
    T[:3, 3] = t
    return T


WORLD_T_CAM0 = _pose((0.3, 1.0, -0.2), 0.7, (0.4, -0.3, 1.1))


def _views():
    """cam_T_world [5,4,4]: view 0 and four views moved and turned a little."""
    out = [np.linalg.inv(WORLD_T_CAM0)]
    for k in range(4):
        d = _pose((np.cos(k), np.sin(k), 0.3), 0.08 + 0.03 * k, (0.12 * np.cos(2.0 * k), 0.08 * np.sin(1.3 * k), -0.05 * k))
        out.append(np.linalg.inv(WORLD_T_CAM0 @ d))
    return np.stack(out)


def grid(nx, ny, x0, x1, y0, y1, z, amp, flip=False):
    """A height field z(x, y) = z + amp sin(3x) cos(2.5y) over [x0,x1] x [y0,y1], nx x ny quads, two triangles each;
    wound counter-clockwise seen from the camera (the -z side) unless flip."""
    xs, ys = np.linspace(x0, x1, nx + 1), np.linspace(y0, y1, ny + 1)
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    Z = z + amp * np.sin(3.0 * X) * np.cos(2.5 * Y)
    v = np.stack([X.ravel(), Y.ravel(), Z.ravel()], -1)
    i = np.arange(nx)[:, None] * (ny + 1) + np.arange(ny)[None, :]
    q = np.stack([i, i + 1, i + ny + 2, i + ny + 1], -1).reshape(-1, 4)   # (x,y) (x,y+1) (x+1,y+1) (x+1,y)
    f = np.concatenate([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], 0)
    # (x,y) -> (x,y+1) -> (x+1,y+1) has its normal along -z: towards a camera at the origin
    return v, (f[:, ::-1] if flip else f)


def room(lo, hi):
    """The 12 triangles of a box seen from inside (normals inward)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c = np.array([[x, y, z] for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    f = []
    centre = (lo + hi) / 2
    for q in quads:
        a, b, cc, d = q
        n = np.cross(c[b] - c[a], c[cc] - c[a])
        if np.dot(n, centre - c[a]) < 0:      # make the normal point into the box
            a, b, cc, d = a, d, cc, b
        f += [(a, b, cc), (a, cc, d)]
    return c, np.asarray(f)


def join(parts):
    vs, fs, base = [], [], 0
    for v, f in parts:
        vs.append(v)
        fs.append(np.asarray(f) + base)
        base += len(v)
    return np.concatenate(vs), np.concatenate(fs)


def scenes():
    out = {}
    # small path: ~5k triangles about a pixel across at 96 x 72, overfilling the frame (no silhouette)
    out["grid"] = (*grid(60, 42, -1.45, 1.45, -1.05, 1.05, 2.0, 0.15), [])
    # large path: a box room from inside; two walls cross the camera plane, one lies behind it
    out["room"] = (*room((-2.0, -1.2, -2.5), (2.1, 1.3, 3.0)), [])
    # both, with an occluder in front: a patch of small triangles hides behind a two-triangle board
    board = grid(1, 1, -0.55, 0.35, -0.3, 0.4, 1.0, 0.0)
    patch = grid(24, 20, -0.75, 0.55, -0.5, 0.6, 1.6, 0.05)
    back = grid(40, 30, -1.9, 1.9, -1.15, 1.25, 2.6, 0.1)
    rv, rf = room((-2.0, -1.2, -2.5), (2.1, 1.3, 3.0))
    v, f = join([(rv, rf), back, patch, board])
    # a patch face is hidden when its three corners project inside the board's outline shrunk by 2 %, seen from the
    # origin: the board is at z = 1, so the outline in x/z, y/z is its own x, y range
    pf = np.arange(len(rf) + len(back[1]), len(rf) + len(back[1]) + len(patch[1]))
    pr = v[f[pf]][..., :2] / v[f[pf]][..., 2:]
    inside = ((pr[..., 0] > -0.55 + 0.02) & (pr[..., 0] < 0.35 - 0.02) & (pr[..., 1] > -0.3 + 0.02) &
              (pr[..., 1] < 0.4 - 0.02)).all(1)
    out["occluder"] = (v, f, pf[inside])
    # near clipping: a floor triangle that passes behind the camera, a far wall behind its tip
    floor = (np.array([[-3.0, 0.8, -2.0], [3.0, 0.8, -2.0], [0.2, 0.75, 6.0]]), np.array([[0, 1, 2]]))
    wall = grid(1, 1, -6.0, 6.0, -5.0, 5.0, 7.0, 0.0)
    out["near"] = (*join([floor, wall]), [])
    # junk mixed in: NaN and infinite vertices, zero area (repeated index, coincident and collinear corners), wholly
    # off screen, wholly behind the camera
    gv, gf = grid(20, 15, -0.7, 0.6, -0.45, 0.5, 1.8, 0.1)   # ends inside the frame: pixels beside it stay empty
    jv = np.array([[np.nan, 0.0, 1.5], [0.1, 0.1, 1.5], [0.2, -0.1, 1.5], [np.inf, 0.0, 1.2],
                   [0.0, 0.0, 1.0], [0.3, 0.3, 1.0], [0.6, 0.6, 1.0],
                   [30.0, 0.0, 2.0], [31.0, 0.0, 2.0], [30.0, 1.0, 2.0],
                   [0.0, 0.0, -1.0], [0.5, 0.0, -1.5], [0.0, 0.5, -2.0],
                   [-0.2, 0.2, 1.2], [0.1, -0.3, 1.3], [0.3, 0.2, 1.25]])
    jf = np.array([[0, 1, 2], [1, 3, 2], [4, 5, 6], [4, 4, 5], [1, 1, 1], [7, 8, 9], [10, 11, 12], [13, 14, 15],
                   [2, 1, 0]])
    v, f = join([(gv, gf), (jv, jf)])
    order = np.random.default_rng(5).permutation(len(f))   # junk faces between the good ones
    out["junk"] = (v, f[order], [])
    return out


def main():
    T = _views()
    R0, t0 = WORLD_T_CAM0[:3, :3], WORLD_T_CAM0[:3, 3]
    for name, (v, f, hidden) in scenes().items():
        with np.errstate(all="ignore"):
            vw = v @ R0.T + t0
        path = os.path.join(HERE, f"raster_{name}.npz")
        np.savez_compressed(path, vertices=vw.astype(np.float32), faces=f.astype(np.int32),
                            cam_T_world=T.astype(np.float32), hidden=np.asarray(hidden, np.int32))
        print(f"{path}: {len(vw)} vertices, {len(f)} faces, {len(hidden)} hidden, {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
