"""Numpy restatement of the depth metrics rules of include/simplerecon_hip.h ("depth metrics"): fp32 per-pixel terms
in the reference's order, fp64 sums, the batched (per frame, nanmean) and the pooled (plain mean) rules."""
import numpy as np

KEYS = ("abs_diff", "abs_rel", "sq_rel", "rmse", "rmse_log", "a5", "a10", "a25", "a0", "a1", "a2", "a3")
THRESH = np.array([1.05, 1.1, 1.25, 1.5625, 1.953125], dtype=np.float32)


def nearest_index(n_in, n_out):
    """F.interpolate(mode="nearest") source index of every output position along one axis."""
    dst = np.arange(n_out)
    if n_in == n_out:
        return dst
    if n_out == 2 * n_in:
        return dst >> 1
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(dst.astype(np.float32) * scale).astype(np.int64), n_in - 1)


def upsample_nearest(pred_bhw, H, W):
    pred = np.asarray(pred_bhw, dtype=np.float32)
    iy, ix = nearest_index(pred.shape[-2], H), nearest_index(pred.shape[-1], W)
    return pred[:, iy][:, :, ix]


def _sums(gt, pred):
    """fp64 totals of one selection of valid pixels: n, (sum, count) of the non-NaN terms, threshold counts."""
    gt = np.asarray(gt, dtype=np.float32).ravel()
    pred = np.asarray(pred, dtype=np.float32).ravel()
    with np.errstate(all="ignore"):
        d = gt - pred
        ad = np.abs(d)
        sq = d * d
        lg = np.log(gt) - np.log(pred)
        terms = [ad, ad / gt, sq / gt, sq, lg * lg]
        r1, r2 = gt / pred, pred / gt
        acc = [((r1 < t) & (r2 < t)).sum() for t in THRESH]
    out = {"n": float(gt.size), "acc": [float(a) for a in acc]}
    out["sum"] = [float(t[~np.isnan(t)].astype(np.float64).sum()) for t in terms]
    out["cnt"] = [float((~np.isnan(t)).sum()) for t in terms]
    return out


def _metrics(s, pooled, mult_a):
    n = s["n"]
    with np.errstate(all="ignore"):
        means = []
        for tot, c in zip(s["sum"], s["cnt"]):
            if pooled and c != n:
                means.append(np.nan)
            else:
                means.append(np.float64(tot) / np.float64(c))
        e = [np.float32(means[0]), np.float32(means[1]), np.float32(means[2]), np.float32(np.sqrt(means[3])),
             np.float32(np.sqrt(means[4]))]
        a = [np.float32(np.float64(c) / np.float64(n)) for c in s["acc"]]
    if mult_a:
        a = [x * np.float32(100.0) for x in a]
    vals = e + [a[0], a[1], a[2], a[1], a[2], a[3], a[4]]
    return dict(zip(KEYS, vals))


def batched(gt_bHW, pred_bHW, valid_bHW, mult_a=False):
    """Per-frame metrics (compute_depth_metrics_batched): dict of float32 [B] arrays, plus the valid counts [B]."""
    gt = np.asarray(gt_bHW, dtype=np.float32)
    pred = np.asarray(pred_bHW, dtype=np.float32)
    valid = np.asarray(valid_bHW, dtype=bool)
    rows = [_metrics(_sums(gt[b][valid[b]], pred[b][valid[b]]), False, mult_a) for b in range(gt.shape[0])]
    out = {k: np.array([r[k] for r in rows], dtype=np.float32) for k in KEYS}
    return out, valid.reshape(valid.shape[0], -1).sum(1)


def pooled(gt, pred, mask, mult_a=False):
    """compute_depth_metrics(gt[mask], pred[mask]): dict of float32 scalars."""
    mask = np.asarray(mask, dtype=bool)
    return _metrics(_sums(np.asarray(gt)[mask], np.asarray(pred)[mask]), True, mult_a)


def score(gt_bHW, pred_bhw, min_depth=0.5, mult_a=True):
    """test.py's scoring: nearest upsample, valid = gt > min_depth, the batched rule."""
    gt = np.asarray(gt_bHW, dtype=np.float32)
    up = upsample_nearest(pred_bhw, gt.shape[-2], gt.shape[-1])
    with np.errstate(invalid="ignore"):
        valid = gt > np.float32(min_depth)
    return batched(gt, up, valid, mult_a)
