"""Numpy restatement of the mesh metrics rules of include/simplerecon_hip.h ("mesh metrics"): brute-force nearest
neighbours (fp32 with the header's formula, and fp64), the surface sampler with the same integer hash, and the metric
reduction."""
import numpy as np

KEYS = ("acc", "comp", "chamfer", "precision", "recall", "f_score")
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def nn_fp32(q, p, chunk=2048):
    """(d2 fp32, index) of the header's rule: d2 = (dx*dx + dy*dy) + dz*dz in fp32, the minimum over all targets and
    the smallest index among equal d2 (argmin)."""
    q = np.asarray(q, np.float32)
    p = np.asarray(p, np.float32)
    d2 = np.empty(len(q), np.float32)
    idx = np.empty(len(q), np.int64)
    for s in range(0, len(q), chunk):
        qq = q[s:s + chunk]
        dx = qq[:, None, 0] - p[None, :, 0]
        dy = qq[:, None, 1] - p[None, :, 1]
        dz = qq[:, None, 2] - p[None, :, 2]
        d = (dx * dx + dy * dy) + dz * dz
        i = d.argmin(1)
        idx[s:s + chunk] = i
        d2[s:s + chunk] = d[np.arange(len(qq)), i]
    return d2, idx


def nn_fp64(q, p, chunk=2048):
    q = np.asarray(q, np.float64)
    p = np.asarray(p, np.float64)
    out = np.empty(len(q))
    for s in range(0, len(q), chunk):
        out[s:s + chunk] = np.sqrt(((q[s:s + chunk, None, :] - p[None]) ** 2).sum(-1).min(1))
    return out


def mix64(z):
    z = (np.asarray(z, np.uint64) + np.uint64(0x9E3779B97F4A7C15)) & M64
    z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & M64
    z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & M64
    return z ^ (z >> np.uint64(31))


def sample_surface(vertices, faces, n, seed=0, tol=1e-9):
    """(points [n,3] fp32, face [n], ambiguous [n] bool): the header's sampler with an fp64 np.cumsum of the areas.
    A sample whose CDF position lies within tol (relative to the total) of a face boundary is ambiguous: the kernel's
    fixed-order sum may put it in the neighbouring face."""
    v = np.asarray(vertices, np.float32)
    f = np.asarray(faces, np.int64)
    v64 = v.astype(np.float64)
    cr = np.cross(v64[f[:, 1]] - v64[f[:, 0]], v64[f[:, 2]] - v64[f[:, 0]])
    area = 0.5 * np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])
    cdf = np.cumsum(area)
    total = cdf[-1]
    i = np.arange(n, dtype=np.uint64)
    with np.errstate(over="ignore"):
        s = mix64(np.uint64(seed))
        h = [mix64(s ^ (np.uint64(3) * i + np.uint64(k))) for k in range(3)]
    x = (h[0] >> np.uint64(12)).astype(np.float64) * 2.0 ** -52 * total
    face = np.searchsorted(cdf, x, side="right")
    lo = np.where(face > 0, cdf[np.maximum(face - 1, 0)], 0.0)
    ambiguous = (np.abs(x - lo) <= tol * total) | (np.abs(cdf[face] - x) <= tol * total)
    u = (h[1] >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    w = (h[2] >> np.uint64(40)).astype(np.float32) * np.float32(2.0 ** -24)
    su = np.sqrt(u)
    a, b, c = np.float32(1) - su, su * (np.float32(1) - w), su * w
    tri = f[face]
    pts = (a[:, None] * v[tri[:, 0]] + b[:, None] * v[tri[:, 1]]) + c[:, None] * v[tri[:, 2]]
    return pts.astype(np.float32), face, ambiguous


def metrics(d_pred_to_gt, d_gt_to_pred, threshold):
    """The six metrics from the two distance arrays (fp32), sums in fp64, strict fp32 threshold compare."""
    dp = np.asarray(d_pred_to_gt, np.float32)
    dg = np.asarray(d_gt_to_pred, np.float32) if len(dp) else None
    t = np.float32(threshold)
    with np.errstate(invalid="ignore", divide="ignore"):
        acc = dp.astype(np.float64).sum() / len(dp) if len(dp) else np.nan
        prec = float((dp < t).sum()) / len(dp) if len(dp) else np.nan
        comp = dg.astype(np.float64).sum() / len(dg) if dg is not None else np.inf
        rec = float((dg < t).sum()) / len(dg) if dg is not None else 0.0
    chamfer = (acc + comp) / 2 if len(dp) else np.inf
    f = 2 * prec * rec / (prec + rec) if prec + rec > 0 else 0.0
    return dict(acc=acc, comp=comp, chamfer=chamfer, precision=prec, recall=rec, f_score=f)
