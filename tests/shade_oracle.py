"""Float64 restatement of the mesh shading kernels (simplerecon_amd/csrc/sr_shade.hip): the yardstick of
render.vertex_normals, render.render_color and render.render_normals.  numpy only.  The rules are those of
include/simplerecon_hip.h, section "mesh shading", applied to a given face-id image; nothing is rasterised here.

The model is a stated one (ambient plus Lambert), not pyrender's shader."""
import numpy as np

UNLIT, NORMALS, LAMBERT = 0, 1, 2
SMOOTH, FLAT = 0, 1
DIRECTIONAL, POINT, HEAD = 0, 1, 2


def vertex_normals(verts, faces):
    """[V,3] float64: normalise(sum over the faces at a vertex of (x1 - x0) x (x2 - x0)); faces with an index outside
    [0, V) or a non-finite cross product are skipped; zero where nothing usable touches a vertex."""
    v = np.asarray(verts, np.float64)
    f = np.asarray(faces, np.int64)
    V = len(v)
    ok = ((f >= 0) & (f < V)).all(1)
    f = f[ok]
    with np.errstate(all="ignore"):
        n = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
        fin = np.isfinite(n).all(1)
        f, n = f[fin], n[fin]
        s = np.zeros((V, 3))
        np.add.at(s, f.ravel(), np.repeat(n, 3, axis=0))
        length = np.sqrt((s * s).sum(1))
        good = (length > 0) & np.isfinite(length)
        return np.where(good[:, None], s / np.where(good, length, 1.0)[:, None], 0.0)


def _blend(attr, f, w):
    a = np.asarray(attr, np.float64)[f]                    # [P,3 corners,3]
    return a[:, 0] * w[:, 0:1] + (a[:, 1] * w[:, 1:2] + a[:, 2] * w[:, 2:3])


def _unit(x):
    return x / np.sqrt((x * x).sum(-1, keepdims=True))


def shade(verts, faces, K, cam_T_world, H, W, pixel_offset, face_hw, colors=None, normals=None,
          base_color=(0.6, 0.6, 0.6), background=(1.0, 1.0, 1.0), ambient=0.4, lights=None, shading=LAMBERT,
          normal_mode=SMOOTH):
    """Shades one view from the face-id image face_hw (-1 = empty).  Returns a dict: color [3,H,W] (clamped to [0, 1],
    NaN -> 0; the background where empty), normals [3,H,W] (0 where empty), hit [H,W] bool, weights [H,W,3], point
    [H,W,3] (the hit point P), grazing [H,W] = |n_g . r| for unit vectors, smooth_length [H,W] = |interpolated normal|
    (NaN without normals).  `lights`: [L,8] records (kind, xyz, rgb intensity, unused)."""
    v = np.asarray(verts, np.float64)
    fa = np.asarray(faces, np.int64)
    K = np.asarray(K, np.float64)
    T = np.asarray(cam_T_world, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    lights = np.zeros((0, 8)) if lights is None else np.asarray(lights, np.float64).reshape(-1, 8)
    fid = np.asarray(face_hw, np.int64).ravel()
    hit = (fid >= 0) & (fid < len(fa))
    f = fa[np.where(hit, fid, 0)]
    hit &= ((f >= 0) & (f < len(v))).all(1)
    f = np.where(hit[:, None], f, 0)
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    r = np.stack([(xx.ravel() - (K[0, 2] - pixel_offset)) / K[0, 0], (yy.ravel() - (K[1, 2] - pixel_offset)) / K[1, 1],
                  np.ones(H * W)], -1)
    with np.errstate(all="ignore"):
        X = v[f] @ R.T + t                                 # [P,3 corners,3]
        a, e1, e2 = X[:, 0], X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
        n = np.cross(e1, e2)
        d = (r * n).sum(1)
        an = (a * n).sum(1)
        P = (an / d)[:, None] * r
        u = -(r * np.cross(a, e2)).sum(1) / d
        vv = -(r * np.cross(e1, a)).sum(1) / d
        w = np.clip(np.stack([1.0 - (u + vv), u, vv], -1), 0.0, 1.0)
        w = w / (w[:, 0] + (w[:, 1] + w[:, 2]))[:, None]
        c = np.broadcast_to(np.asarray(base_color, np.float64), (H * W, 3)) if colors is None else _blend(colors, f, w)
        ng = _unit(n)
        ng = np.where(((ng * P).sum(1) > 0)[:, None], -ng, ng)
        nn = ng
        length = np.full(H * W, np.nan)
        if normals is not None:
            m = _blend(normals, f, w) @ R.T
            length = np.sqrt((m * m).sum(1))
            if normal_mode == SMOOTH:
                ns = m / length[:, None]
                ns = np.where((an >= 0)[:, None], -ns, ns)          # back-facing: the rasteriser's c >= 0
                nn = np.where(((length >= 1e-12) & np.isfinite(length))[:, None], ns, ng)
        if shading == NORMALS:
            c = 0.5 * (1.0 + nn)
        elif shading == LAMBERT:
            total = np.zeros((H * W, 3))
            for L in lights:
                kind = int(L[0])
                if kind == DIRECTIONAL:
                    dirn = np.broadcast_to(-(R @ _unit(L[1:4])), (H * W, 3))
                    att = 1.0
                elif kind == POINT:
                    D = (R @ L[1:4] + t) - P
                    d2 = (D * D).sum(1)
                    dirn = D / np.sqrt(d2)[:, None]
                    att = 1.0 / np.maximum(d2, 1e-12)
                elif kind == HEAD:
                    dirn = -_unit(P)
                    att = 1.0
                else:
                    raise ValueError(f"unknown light kind {L[0]}")
                s = np.fmax(0.0, (nn * dirn).sum(1)) * att           # (fmax: a NaN cosine lights nothing)
                total = total + L[4:7][None, :] * s[:, None]
            c = c * (ambient + total)
        c = np.where(np.isnan(c), 0.0, np.clip(c, 0.0, 1.0))
        rhat = _unit(r)
        grazing = np.abs((ng * rhat).sum(1))
    color = np.where(hit[:, None], c, np.asarray(background, np.float64)[None, :])
    nn = np.where(hit[:, None], nn, 0.0)
    return dict(color=color.T.reshape(3, H, W), normals=nn.T.reshape(3, H, W), hit=hit.reshape(H, W),
                weights=w.reshape(H, W, 3), point=P.reshape(H, W, 3), grazing=grazing.reshape(H, W),
                smooth_length=length.reshape(H, W))
