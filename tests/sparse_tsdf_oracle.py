"""numpy restatement of include/simplerecon_hip.h, section "sparse TSDF" (the checker of csrc/sr_sparse_tsdf.hip):
fp64 touch, fp32 integration in the stated operation order, and marching cubes over the blocks in fp32 with
unobserved voxels as NaN, numbered in block order.  The loop tables come from tests/mesh_oracle.py (whose own
marching_cubes rounds values through fp16 and is not used here)."""
import numpy as np

from mesh_oracle import EDGES, FACES, loop_triangles

BLOCK = 16
VOXELS = BLOCK ** 3
KEY_OFFSET = 1 << 20
f32 = np.float32

# local voxel coordinates of l = (lx * 16 + ly) * 16 + lz
_LOCAL = np.stack(np.meshgrid(np.arange(BLOCK), np.arange(BLOCK), np.arange(BLOCK), indexing="ij"), -1).reshape(-1, 3)


def pack(coords):
    b = np.asarray(coords, dtype=np.int64).reshape(-1, 3) + KEY_OFFSET
    return (b[:, 0] << 42) | (b[:, 1] << 21) | b[:, 2]


def unpack(keys):
    k = np.asarray(keys, dtype=np.int64).reshape(-1)
    m = (1 << 21) - 1
    return np.stack([(k >> 42) & m, (k >> 21) & m, k & m], 1) - KEY_OFFSET


def preprocess_depth(depth_hw, max_depth):
    d = np.asarray(depth_hw, dtype=np.float32).copy()
    with np.errstate(invalid="ignore"):
        d[d > f32(max_depth)] = 0
    return d


def touch(depth_hw, K44, T44, sdf_trunc, unit):
    """Sorted unique keys of the blocks a (preprocessed) depth map touches: pixels on the 4x4 grid with d > 0, fp64."""
    K = np.asarray(K44, dtype=np.float32).astype(np.float64)
    M = np.linalg.inv(np.asarray(T44, dtype=np.float32).astype(np.float64))
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    h, w = depth_hw.shape
    vv, uu = np.meshgrid(np.arange(0, h, 4), np.arange(0, w, 4), indexing="ij")
    d = depth_hw[vv, uu].astype(np.float64)
    ok = d > 0
    u, v, d = uu[ok].astype(np.float64), vv[ok].astype(np.float64), d[ok]
    x, y, z = ((u - cx) * d) / fx, ((v - cy) * d) / fy, d
    lo, hi = [], []
    fin = np.ones(len(d), dtype=bool)
    with np.errstate(invalid="ignore"):
        for a in range(3):
            p = ((M[a, 0] * x + M[a, 1] * y) + M[a, 2] * z) + M[a, 3]
            lo.append(np.floor((p - sdf_trunc) / unit))
            hi.append(np.floor((p + sdf_trunc) / unit))
            fin &= np.isfinite(lo[-1]) & np.isfinite(hi[-1])
    keys = []
    for k in range(8):
        b = np.stack([(hi if (k >> a) & 1 else lo)[a][fin] for a in range(3)], 1)
        inr = ((b >= -KEY_OFFSET) & (b < KEY_OFFSET)).all(1)
        keys.append(pack(b[inr].astype(np.int64)))
    return np.unique(np.concatenate(keys)) if keys else np.zeros(0, dtype=np.int64)


class Volume:
    """Blocks: key -> [5, 4096] fp32 (tsdf, weight, red, green, blue)."""

    def __init__(self, voxel_length, sdf_trunc, max_depth):
        self.vl = float(voxel_length)
        self.trunc = float(sdf_trunc)
        self.max_depth = float(max_depth)
        self.unit = BLOCK * self.vl
        self.blocks = {}

    def arrays(self):
        """(keys [N] sorted, tsdf [N,4096], weight [N,4096], rgb [N,3,4096])."""
        keys = np.array(sorted(self.blocks), dtype=np.int64)
        data = np.stack([self.blocks[k] for k in keys]) if len(keys) else np.zeros((0, 5, VOXELS), np.float32)
        return keys, data[:, 0], data[:, 1], data[:, 2:5]

    def integrate(self, depth_bhw, K_b44, T_b44, color_b3hw=None):
        for f in range(len(depth_bhw)):
            self.integrate_frame(depth_bhw[f], K_b44[f], T_b44[f], None if color_b3hw is None else color_b3hw[f])

    def integrate_frame(self, depth_hw, K44, T44, color_3hw=None):
        depth = preprocess_depth(depth_hw, self.max_depth)
        keys = touch(depth, K44, T44, self.trunc, self.unit)
        if len(keys) == 0:
            return
        for k in keys:
            if k not in self.blocks:
                self.blocks[k] = np.zeros((5, VOXELS), dtype=np.float32)
        data = np.stack([self.blocks[k] for k in keys])
        data = integrate_blocks(data, unpack(keys), depth, K44, T44, color_3hw, self.vl, self.trunc)
        for i, k in enumerate(keys):
            self.blocks[k] = data[i]


def integrate_blocks(data, coords, depth, K44, T44, color_3hw, vl, trunc):
    """One frame on the blocks it touched: data [n,5,4096] fp32, coords [n,3]; returns the updated data."""
    K = np.asarray(K44, dtype=np.float32)
    T = np.asarray(T44, dtype=np.float32)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    h, w = depth.shape
    vl, tr = f32(vl), f32(trunc)
    g = (coords[:, None, :] * BLOCK + _LOCAL[None]).astype(np.int64)            # [n,4096,3]
    c = (g.astype(np.float32) + f32(0.5)) * vl
    x, y, z = c[..., 0], c[..., 1], c[..., 2]
    px = ((T[0, 0] * x + T[0, 1] * y) + T[0, 2] * z) + T[0, 3]
    py = ((T[1, 0] * x + T[1, 1] * y) + T[1, 2] * z) + T[1, 3]
    pz = ((T[2, 0] * x + T[2, 1] * y) + T[2, 2] * z) + T[2, 3]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        ok = ~(pz <= 0)
        uf = ((px * fx) / pz + cx) + f32(0.5)
        vf = ((py * fy) / pz + cy) + f32(0.5)
        ok &= (uf >= f32(0.0001)) & (uf < f32(w) - f32(0.0001)) & (vf >= f32(0.0001)) & (vf < f32(h) - f32(0.0001))
        u = np.where(ok, uf, 0).astype(np.int32)
        v = np.where(ok, vf, 0).astype(np.int32)
        D = depth[v, u]
        ok &= ~(D <= 0)
        a = (u.astype(np.float32) - cx) / fx
        b = (v.astype(np.float32) - cy) / fy
        sdf = (D - pz) * np.sqrt((f32(1) + a * a) + b * b)
        ok &= sdf > -tr
        tn = np.minimum(f32(1), sdf / tr)
    out = data.copy()
    W = data[:, 1]
    W1 = W + f32(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        out[:, 0] = np.where(ok, (data[:, 0] * W + tn) / W1, data[:, 0])
        for ch in range(3):
            col = f32(178) if color_3hw is None else np.asarray(color_3hw[ch])[v, u].astype(np.float32)
            out[:, 2 + ch] = np.where(ok, (data[:, 2 + ch] * W + col) / W1, data[:, 2 + ch])
    out[:, 1] = np.where(ok, W1, W)
    return out.astype(np.float32)


def extract_mesh(keys, tsdf, weight, rgb, voxel_length):
    """Marching cubes over the blocks.  keys [N] sorted; tsdf / weight [N,4096] (or [N,16,16,16]); rgb [N,3,4096].
    Returns (vertices [V,3] f32, faces [F,3] int32, colors [V,3] f32, positions [V,3] f32 in global voxel units,
    owner [V,4] int64: the global voxel index and axis of each vertex's edge)."""
    keys = np.asarray(keys, dtype=np.int64)
    N = len(keys)
    empty = (np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), np.zeros((0, 3), np.float32),
             np.zeros((0, 3), np.float32), np.zeros((0, 4), np.int64))
    if N == 0:
        return empty
    tsdf = np.asarray(tsdf, np.float32).reshape(N, VOXELS)
    weight = np.asarray(weight, np.float32).reshape(N, VOXELS)
    rgb = np.asarray(rgb, np.float32).reshape(N, 3, VOXELS)
    coords = unpack(keys)
    off = coords.min(0) * BLOCK
    dims = (coords.max(0) - coords.min(0) + 1) * BLOCK
    X, Y, Z = (int(d) for d in dims)
    val = np.full((X, Y, Z), np.nan, dtype=np.float32)
    col = np.zeros((3, X, Y, Z), dtype=np.float32)
    rank = np.full((X // BLOCK, Y // BLOCK, Z // BLOCK), -1, dtype=np.int64)
    for n in range(N):
        i0, j0, k0 = (coords[n] * BLOCK - off)
        vals = np.where(weight[n] != 0, np.clip(tsdf[n], f32(-1), f32(1)), np.float32(np.nan))
        val[i0:i0 + BLOCK, j0:j0 + BLOCK, k0:k0 + BLOCK] = vals.reshape(BLOCK, BLOCK, BLOCK)
        col[:, i0:i0 + BLOCK, j0:j0 + BLOCK, k0:k0 + BLOCK] = rgb[n].reshape(3, BLOCK, BLOCK, BLOCK)
        rank[i0 // BLOCK, j0 // BLOCK, k0 // BLOCK] = n
    lvl = f32(0)
    below = val < lvl
    nan = np.isnan(val)

    def order_key(idx, a):
        """Sort key of a voxel's edge (or cube: a = 0): block rank, local index, axis."""
        r = rank[idx[:, 0] // BLOCK, idx[:, 1] // BLOCK, idx[:, 2] // BLOCK]
        loc = ((idx[:, 0] % BLOCK) * BLOCK + idx[:, 1] % BLOCK) * BLOCK + idx[:, 2] % BLOCK
        return (r * VOXELS + loc) * 3 + a

    # ---- vertices
    okeys, pos, cols, owner = [], [], [], []
    dense_key = []
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        cross = (below[lo] != below[hi]) & ~nan[lo] & ~nan[hi]
        idx = np.stack(np.nonzero(cross), 1)
        v0, v1 = val[lo][cross], val[hi][cross]
        t = (lvl - v0) / (v1 - v0)
        gidx = idx + off[None]
        p = gidx.astype(np.float32)
        p[:, a] = p[:, a] + t
        c0 = col[(slice(None),) + lo][:, cross].T
        c1 = col[(slice(None),) + hi][:, cross].T
        okeys.append(order_key(idx, a))
        dense_key.append(((idx[:, 0] * Y + idx[:, 1]) * Z + idx[:, 2]) * 3 + a)
        pos.append(p)
        cols.append((c0 + t[:, None] * (c1 - c0)) / f32(255))
        owner.append(np.concatenate([gidx, np.full((len(idx), 1), a)], 1))
    allk = np.concatenate(okeys)
    order = np.argsort(allk, kind="stable")
    vpos = np.concatenate(pos)[order].astype(np.float32)
    vcol = np.concatenate(cols)[order].astype(np.float32)
    vown = np.concatenate(owner)[order]
    dkeys = np.concatenate(dense_key)[order]
    dsort = np.argsort(dkeys, kind="stable")          # dense edge key -> vertex id
    verts = ((vpos + f32(0.5)) * f32(voxel_length)).astype(np.float32)
    # ---- cubes
    cv = np.stack([val[(c & 1):X - 1 + (c & 1), (c >> 1 & 1):Y - 1 + (c >> 1 & 1), (c >> 2 & 1):Z - 1 + (c >> 2 & 1)]
                   for c in range(8)], -1).reshape(-1, 8)
    cidx = np.stack(np.meshgrid(np.arange(X - 1), np.arange(Y - 1), np.arange(Z - 1), indexing="ij"), -1).reshape(-1, 3)
    up = ~(cv < lvl)
    config = (up.astype(np.int64) << np.arange(8)).sum(1)
    keep = (config != 0) & (config != 255) & ~np.isnan(cv).any(1)
    cv, cidx, config, up = cv[keep], cidx[keep], config[keep], up[keep]
    dec = np.zeros(len(cv), dtype=np.int64)
    for f, (cs, _) in enumerate(FACES):
        u = up[:, cs]
        amb = (u[:, 0] == u[:, 2]) & (u[:, 1] == u[:, 3]) & (u[:, 0] != u[:, 1])
        d = cv[:, cs] - lvl
        a_pair = np.where(u[:, 0], d[:, 0] * d[:, 2], d[:, 1] * d[:, 3])
        b_pair = np.where(u[:, 0], d[:, 1] * d[:, 3], d[:, 0] * d[:, 2])
        dec |= (amb & (a_pair >= b_pair)).astype(np.int64) << f
    key = config | dec << 8
    cube_order = order_key(cidx, 0) // 3
    face_rows, face_order = [], []
    for k in np.unique(key):
        sel = np.nonzero(key == k)[0]
        tris = loop_triangles(int(k & 255), int(k >> 8))
        if not tris:
            continue
        base = cidx[sel]
        ids = np.empty((len(sel), len(tris), 3), dtype=np.int64)
        for t_i, tri in enumerate(tris):
            for m, e in enumerate(tri):
                c, a = EDGES[e]
                own = base + np.array([c & 1, c >> 1 & 1, c >> 2 & 1])
                dk = ((own[:, 0] * Y + own[:, 1]) * Z + own[:, 2]) * 3 + a
                ids[:, t_i, m] = dsort[np.searchsorted(dkeys[dsort], dk)]
        p = vpos[ids]
        eq = lambda i, j: (p[:, :, i] == p[:, :, j]).all(-1)  # noqa: E731
        good = ~(eq(0, 1) | eq(1, 2) | eq(0, 2))
        n_i, t_i = np.nonzero(good)
        face_rows.append(ids[n_i, t_i])
        face_order.append(cube_order[sel][n_i] * 16 + t_i)
    if face_rows:
        rows, fo = np.concatenate(face_rows), np.concatenate(face_order)
        faces = rows[np.argsort(fo, kind="stable")].astype(np.int32)
    else:
        faces = np.zeros((0, 3), dtype=np.int32)
    return verts, faces, vcol, vpos, vown
