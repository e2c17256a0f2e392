"""fp64 numpy restatement of the point-cloud fusion rules of include/simplerecon_hip.h ("point-cloud fusion"), with
what the comparison rule needs to know: which decisions sit within rounding distance of a threshold, and how far the
averaged point could move if another admissible texel were read."""
import numpy as np

EPS_PX = 5e-3      # a coordinate this close to a .5 boundary may round to either neighbour
EPS_M = 1e-5       # decision margins below this (metres or pixels) are ambiguous


def frame_constants(P, K):
    P = np.asarray(P, np.float64)
    K = np.asarray(K, np.float64)[..., :3, :3]
    return P, K, np.linalg.inv(K), np.linalg.inv(P)


def fuse_frame(depths, P, K, r, z_thresh, pixels=None, eps_px=EPS_PX, eps_m=EPS_M):
    """Reference frame r against all others (ascending).  `pixels`: flat pixel indices (default all).
    Returns dict of n [P], avg [P,3], amb [P] bool, tol [P] (the spread term of the comparison rule)."""
    D = np.asarray(depths, np.float64)
    N, h, w = D.shape
    P, K, Kinv, Pinv = frame_constants(P, K)
    pix = np.arange(h * w) if pixels is None else np.asarray(pixels)
    v, u = np.divmod(pix, w)
    d = D[r].reshape(-1)[pix]
    cam = Kinv[r] @ np.stack([u * d, v * d, d])
    X = Pinv[r, :3, :3] @ cam + Pinv[r, :3, 3:]
    n = np.zeros(len(pix), np.int64)
    acc = X.copy()
    amb = np.zeros(len(pix), bool)
    spread = np.zeros(len(pix))
    with np.errstate(all="ignore"):
        for s in range(N):
            if s == r:
                continue
            R, t = P[s, :3, :3], P[s, :3, 3:]
            q = K[s] @ (R @ X + t)
            z = q[2]
            x, y = q[0] / z, q[1] / z
            # decision terms: (robust value, ambiguous)
            terms = [(z > 1e-4, np.abs(z - 1e-4) < eps_m)]
            for c, hi in ((x, w - 1), (y, h - 1)):
                terms.append((c >= 0, np.abs(c) < eps_m))
                terms.append((c <= hi, np.abs(c - hi) < eps_m))
            # admissible texels (grid_sample nearest, align_corners=True: round half to even)
            def texels(c, size):
                c0 = np.clip(np.nan_to_num(np.rint(c), nan=0, posinf=size - 1, neginf=0), 0, size - 1).astype(np.int64)
                fl = np.floor(np.nan_to_num(c, nan=0, posinf=0, neginf=0))
                near = np.abs(np.nan_to_num(c, nan=0, posinf=0, neginf=0) - fl - 0.5) < eps_px
                a = np.clip(fl, 0, size - 1).astype(np.int64)
                b = np.clip(fl + 1, 0, size - 1).astype(np.int64)
                return [c0, np.where(near, a, c0), np.where(near, b, c0)]
            xs, ys = texels(x, w), texels(y, h)
            zs = [D[s][ys[j], xs[i]] for (i, j) in ((0, 0), (1, 1), (1, 2), (2, 1), (2, 2))]
            Ys = [R.T @ (Kinv[s] @ np.stack([x * zz, y * zz, zz]) - t) for zz in zs]
            cons = [np.abs(z - zz) < z_thresh for zz in zs]
            cons_amb = np.abs(np.abs(z - zs[0]) - z_thresh) < eps_m
            for k in range(1, len(zs)):
                cons_amb |= cons[k] != cons[0]
                cons_amb |= np.abs(np.abs(z - zs[k]) - z_thresh) < eps_m
            terms.append((cons[0], cons_amb))
            robust_false = np.zeros(len(pix), bool)
            any_amb = np.zeros(len(pix), bool)
            for val, am in terms:
                robust_false |= ~val & ~am
                any_amb |= am
            ok = ~robust_false & ~any_amb
            for val, _ in terms:
                ok &= val
            amb |= ~robust_false & any_amb
            good = ok & ~np.isnan(Ys[0]).any(0)
            n += ok
            acc += np.where(good, np.nan_to_num(Ys[0]), 0.0)
            sp = np.zeros(len(pix))
            for k in range(1, len(Ys)):
                sp = np.maximum(sp, np.nan_to_num(np.abs(Ys[k] - Ys[0]), nan=np.inf).max(0))
            spread += np.where(ok, sp, 0.0)
    return dict(n=n, avg=(acc / (n + 1)).T, amb=amb, tol=spread / (n + 1))


def fuse_scene(depths, P, K, z_thresh, pixels_per_frame=None, **kw):
    """All frames; returns stacked arrays [N, P...]."""
    N = np.asarray(depths).shape[0]
    out = [fuse_frame(depths, P, K, r, z_thresh, None if pixels_per_frame is None else pixels_per_frame[r], **kw)
           for r in range(N)]
    return {k: np.stack([o[k] for o in out]) for k in out[0]}


def compare(orc, thresh, got_valid, got_pts, got_rgb, images, got_n=None, max_amb=0.005, atol=2e-5):
    """The comparison rule.  orc: fuse_scene output over all pixels; got_*: a fused result (points listed frame by
    frame, row-major).  Raises AssertionError with a description on mismatch; returns the ambiguous fraction."""
    N, h, w = got_valid.shape
    amb = orc["amb"].reshape(N, h, w)
    keep = (orc["n"] >= thresh).reshape(N, h, w)
    frac = float(amb.mean())
    assert frac < max_amb, f"{frac:.4%} of pixels are ambiguous"
    bad = (keep != got_valid) & ~amb
    assert not bad.any(), f"{int(bad.sum())} unambiguous keep decisions differ, first at {np.argwhere(bad)[0]}"
    if got_n is not None:
        badn = (orc["n"].reshape(N, h, w) != got_n) & ~amb
        assert not badn.any(), f"{int(badn.sum())} unambiguous counts differ, first at {np.argwhere(badn)[0]}"
    flat = np.flatnonzero(got_valid.reshape(-1))
    assert len(flat) == len(got_pts)
    sel = ~amb.reshape(-1)[flat]
    want = orc["avg"].reshape(-1, 3)[flat[sel]]
    tol = atol + orc["tol"].reshape(-1)[flat[sel]]
    err = np.abs(np.asarray(got_pts, np.float64)[sel] - want).max(1) if sel.any() else np.zeros(0)
    assert (err <= tol).all(), f"averaged points off by up to {err.max():.3e} (tolerance there {tol[err.argmax()]:.3e})"
    if images is not None:
        assert np.array_equal(np.asarray(got_rgb), np.asarray(images).reshape(-1, 3)[flat])
    return frac


def voxel_down_sample(points, colors, voxel_size):
    """open3d's voxel_down_sample rules in fp64; returns (points fp32, colours uint8 or None, keys int64)."""
    p = np.asarray(points, np.float32).astype(np.float64)
    mn = p.min(0) - voxel_size * 0.5
    idx = np.floor((p - mn) / voxel_size).astype(np.int64)
    assert (idx < 2 ** 21).all()
    key = (idx[:, 0] << 42) | (idx[:, 1] << 21) | idx[:, 2]
    order = np.argsort(key, kind="stable")
    sk = key[order]
    uk, start = np.unique(sk, return_index=True)
    cnt = np.diff(np.append(start, len(sk)))
    pts = np.stack([np.array([p[order[a:a + c]].sum(0) for a, c in zip(start, cnt)]).reshape(-1, 3)])[0]
    out = (pts / cnt[:, None]).astype(np.float32)
    col = None
    if colors is not None:
        cs = np.add.reduceat(np.asarray(colors, np.int64)[order], start, axis=0)
        col = ((cs + cnt[:, None] // 2) // cnt[:, None]).astype(np.uint8)
    return out, col, uk


def torch_fuse(depths, P, K, z_thresh, n_consistent_thresh, batch=100):
    """The same rules as batched fp32 torch on any device (the reference's formulation: all sources of a batch at
    once, grid_sample for the texel): a timing baseline, not a checker.  Returns (points [M,3], valid [N,h,w])."""
    import torch
    import torch.nn.functional as F
    N, h, w = depths.shape
    dev = depths.device
    P, K = P.to(dev, torch.float32), K.to(dev, torch.float32)[:, :3, :3]
    Kinv, Pinv = torch.linalg.inv(K), torch.linalg.inv(P)
    vv, uu = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32),
                            torch.arange(w, device=dev, dtype=torch.float32), indexing="ij")
    uv1 = torch.stack([uu, vv, torch.ones_like(uu)]).reshape(3, -1)
    out_p, out_v = [], []
    for r in range(N):
        X = Pinv[r, :3, :3] @ (Kinv[r] @ (uv1 * depths[r].reshape(1, -1))) + Pinv[r, :3, 3:]
        acc, n = X.clone(), torch.zeros(h * w, device=dev, dtype=torch.int32)
        src = torch.tensor([s for s in range(N) if s != r], device=dev, dtype=torch.long)
        for b in range(0, len(src), batch):
            s = src[b:b + batch]
            q = K[s] @ (P[s, :3, :3] @ X + P[s, :3, 3:])
            z = q[:, 2]
            x, y = q[:, 0] / z, q[:, 1] / z
            inb = (z > 1e-4) & (x >= 0) & (x <= w - 1) & (y >= 0) & (y <= h - 1)
            grid = torch.stack([x / (w - 1) * 2 - 1, y / (h - 1) * 2 - 1], -1)[:, :, None]
            zs = F.grid_sample(depths[s][:, None], grid, mode="nearest", align_corners=True)[:, 0, :, 0]
            ok = inb & ((z - zs).abs() < z_thresh)
            Y = P[s, :3, :3].transpose(1, 2) @ (Kinv[s] @ (torch.stack([x, y, torch.ones_like(x)], 1) * zs[:, None])
                                                  - P[s, :3, 3:])
            ok_y = ok & ~torch.isnan(Y).any(1)
            n += ok.sum(0, dtype=torch.int32)
            acc += torch.where(ok_y[:, None], Y.nan_to_num(), 0).sum(0)
        keep = n >= n_consistent_thresh
        out_p.append((acc / (n + 1)).T[keep])
        out_v.append(keep.reshape(h, w))
    return torch.cat(out_p), torch.stack(out_v)
