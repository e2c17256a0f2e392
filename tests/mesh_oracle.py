"""numpy marching cubes with the rules of include/simplerecon_hip.h, section "mesh extraction" (the checker of
csrc/sr_mesh.hip).  Vertices are computed for all edges at once; triangles come from one loop table per
(cube configuration, face decisions) key, applied to every cube with that key."""
import functools

import numpy as np

# cube corners c = dx | dy << 1 | dz << 2; edges numbered by (owning corner in (dx, dy, dz) lexicographic order, axis)
EDGES = []
for _key in range(8):
    _c = (_key >> 2 & 1) | (_key >> 1 & 1) << 1 | (_key & 1) << 2
    EDGES += [(_c, a) for a in range(3) if not (_c >> a) & 1]
_EDGE_ID = {e: n for n, e in enumerate(EDGES)}


def _edge(c0, c1):
    return _EDGE_ID[(min(c0, c1), (1, 2, 4).index(c0 ^ c1))]


# faces: corners counter-clockwise seen from outside the cube, and the edge from corner k to corner k+1
FACES = []
for _n in range(3):
    _u, _w = (_n + 1) % 3, (_n + 2) % 3
    for _s in range(2):
        _cyc = [(0, 0), (1, 0), (1, 1), (0, 1)] if _s else [(0, 0), (0, 1), (1, 1), (1, 0)]
        _cs = [_s << _n | pu << _u | pw << _w for pu, pw in _cyc]
        FACES.append((_cs, [_edge(_cs[k], _cs[(k + 1) % 4]) for k in range(4)]))


@functools.lru_cache(maxsize=None)
def loop_triangles(config, decisions):
    """Triangles (edge triples, output order) of a cube whose above corners are the bits of `config`; bit f of
    `decisions`: on ambiguous face f the above corners are joined."""
    up = [(config >> c) & 1 for c in range(8)]
    nxt = {}
    for f, (cs, es) in enumerate(FACES):
        u = [up[c] for c in cs]
        ncross = sum(u[k] != u[(k + 1) % 4] for k in range(4))
        for k in range(4):
            if not (u[k] and not u[(k + 1) % 4]):
                continue
            if ncross == 2:
                end = next(es[m] for m in range(4) if not u[m] and u[(m + 1) % 4])
            else:
                end = es[(k + 1) % 4] if (decisions >> f) & 1 else es[(k + 3) % 4]
            nxt[es[k]] = end
    tris, seen = [], set()
    for e0 in sorted(nxt):
        if e0 in seen:
            continue
        seen.add(e0)
        b = nxt[e0]
        seen.add(b)
        c = nxt[b]
        while c != e0:
            seen.add(c)
            tris.append((e0, b, c))
            b, c = c, nxt[c]
    return tuple(tris)


def marching_cubes(values, level=0.0, origin=(0.0, 0.0, 0.0), scale=1.0, normals=True):
    """values: [X,Y,Z] fp16 (or anything cast to fp16).  Returns (vertices [V,3] f32, faces [F,3] int32,
    normals [V,3] f32 or None, voxel-unit positions [V,3] f32)."""
    v = np.clip(np.asarray(values, dtype=np.float16).astype(np.float32), -1.0, 1.0)
    X, Y, Z = v.shape
    lvl = np.float32(level)
    below = v < lvl
    nan = np.isnan(v)
    # ---- vertices: every crossing edge, ordered by (linear voxel index, axis)
    lin = np.arange(X * Y * Z, dtype=np.int64).reshape(X, Y, Z)
    keys, pos, tpar, ends = [], [], [], []
    for a in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[a], hi[a] = slice(0, -1), slice(1, None)
        lo, hi = tuple(lo), tuple(hi)
        cross = (below[lo] != below[hi]) & ~nan[lo] & ~nan[hi]
        idx = np.nonzero(cross)
        v0, v1 = v[lo][idx], v[hi][idx]
        t = (lvl - v0) / (v1 - v0)
        p = np.stack([i.astype(np.float32) for i in idx], 1)
        p[:, a] = p[:, a] + t
        keys.append(lin[lo][idx] * 3 + a)
        pos.append(p)
        tpar.append(t)
        ends.append((np.stack(idx, 1), a))
    order = np.argsort(np.concatenate(keys), kind="stable")
    vkeys = np.concatenate(keys)[order]
    vpos = np.concatenate(pos)[order].astype(np.float32)
    o = np.asarray(origin, dtype=np.float32)
    verts = (o[None] + vpos * np.float32(scale)).astype(np.float32)
    norms = None
    if normals:
        g = np.stack(np.gradient(v.astype(np.float32), axis=(0, 1, 2)), -1).astype(np.float32)
        nl = []
        for (idx, a), t in zip(ends, tpar):
            d = np.zeros(3, dtype=np.int64)
            d[a] = 1
            g0 = g[idx[:, 0], idx[:, 1], idx[:, 2]]
            g1 = g[idx[:, 0] + d[0], idx[:, 1] + d[1], idx[:, 2] + d[2]]
            nl.append(g0 + t[:, None] * (g1 - g0))
        n = np.concatenate(nl)[order].astype(np.float32)
        ln = np.sqrt((n * n).sum(1, dtype=np.float32)).astype(np.float32)
        norms = np.where(ln[:, None] > 0, n / np.where(ln > 0, ln, 1)[:, None], 0).astype(np.float32)
    # ---- cubes
    cv = np.stack([v[(c & 1):X - 1 + (c & 1), (c >> 1 & 1):Y - 1 + (c >> 1 & 1), (c >> 2 & 1):Z - 1 + (c >> 2 & 1)]
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
        # above corners: 0, 2 if corner 0 is above, else 1, 3
        a_pair = np.where(u[:, 0], d[:, 0] * d[:, 2], d[:, 1] * d[:, 3])
        b_pair = np.where(u[:, 0], d[:, 1] * d[:, 3], d[:, 0] * d[:, 2])
        dec |= (amb & (a_pair >= b_pair)).astype(np.int64) << f
    key = config | dec << 8
    cube_lin = (cidx[:, 0].astype(np.int64) * Y + cidx[:, 1]) * Z + cidx[:, 2]
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
                vk = ((own[:, 0] * Y + own[:, 1]) * Z + own[:, 2]) * 3 + a
                ids[:, t_i, m] = np.searchsorted(vkeys, vk)
        p = vpos[ids]                                          # [n, T, 3, 3]
        eq = lambda i, j: (p[:, :, i] == p[:, :, j]).all(-1)  # noqa: E731
        good = ~(eq(0, 1) | eq(1, 2) | eq(0, 2))
        n_i, t_i = np.nonzero(good)
        face_rows.append(ids[n_i, t_i])
        face_order.append(cube_lin[sel][n_i] * 16 + t_i)
    if face_rows:
        rows, fo = np.concatenate(face_rows), np.concatenate(face_order)
        faces = rows[np.argsort(fo, kind="stable")].astype(np.int32)
    else:
        faces = np.zeros((0, 3), dtype=np.int32)
    return verts, faces, norms, vpos


def canonical_faces(faces):
    """Rotates every triangle so its smallest index comes first (keeps the winding) and sorts the rows."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    r = np.argmin(f, 1)
    f = np.stack([f[np.arange(len(f)), (r + s) % 3] for s in range(3)], 1)
    return f[np.lexsort(f.T[::-1])]
