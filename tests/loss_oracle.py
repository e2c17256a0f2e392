"""fp64 torch restatement of the training losses (include/simplerecon_hip.h, section "training losses"; the reference's
losses.py, NormalGenerator and DepthModel.compute_losses).  Test infrastructure: runs on CPU tensors, differentiates
with torch autograd, and reports which multi-view decisions lie within rounding distance of the 1.05 threshold or of a
.5 texel boundary (there the fp32 kernel and the fp32 reference may legitimately disagree)."""
import math

import torch
import torch.nn.functional as F

D = torch.float64
KEYS = ("loss", "si_loss", "grad_loss", "abs_loss", "normals_loss", "ms_loss", "inv_abs_loss", "log_l1_loss", "mv_loss")


def blur_pool2d(x):
    k = torch.tensor([1.0, 2.0, 1.0], dtype=x.dtype, device=x.device)
    k = (k[:, None] * k[None, :] / 16.0).view(1, 1, 3, 3).repeat(x.shape[1], 1, 1, 1)
    return F.conv2d(x, k, padding=1, stride=2, groups=x.shape[1])


def spatial_gradient(x):
    """[B,C,h,w] -> [B,C,2,h,w]: Sobel / 8, replicate borders, gx first."""
    sx = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]], dtype=x.dtype, device=x.device) / 8.0
    k = torch.stack([sx, sx.t()]).unsqueeze(1).repeat(x.shape[1], 1, 1, 1)
    xp = F.pad(x, (1, 1, 1, 1), mode="replicate")
    return F.conv2d(xp, k, groups=x.shape[1]).view(x.shape[0], x.shape[1], 2, x.shape[2], x.shape[3])


def gaussian_blur2d(x):
    t = torch.arange(-2, 3, dtype=x.dtype, device=x.device)
    g = torch.exp(-t * t / 8.0)
    g = g / g.sum()
    k = (g[:, None] * g[None, :]).view(1, 1, 5, 5).repeat(x.shape[1], 1, 1, 1)
    return F.conv2d(F.pad(x, (2, 2, 2, 2), mode="reflect"), k, groups=x.shape[1])


def pix_rays(invK, h, w):
    dt = dict(dtype=D, device=invK.device)
    ys, xs = torch.meshgrid(torch.arange(h, **dt), torch.arange(w, **dt), indexing="ij")
    pix = torch.stack([xs.flatten() + 0.5, ys.flatten() + 0.5, torch.ones(h * w, **dt)], 0)
    return invK[:, :3, :3].to(D) @ pix   # [B,3,N]


def normals(depth, invK):
    B, _, h, w = depth.shape
    s = gaussian_blur2d(depth.to(D))
    pts = (s.flatten(2) * pix_rays(invK, h, w)).view(B, 3, h, w)
    g = spatial_gradient(pts)
    return F.normalize(torch.cross(g[:, :, 0], g[:, :, 1], dim=1), dim=1, eps=1e-12)


def normals_loss(ngt, npred):
    m = ngt.isfinite().all(1, keepdim=True) & npred.isfinite().all(1, keepdim=True)
    dot = 0.5 * (1.0 - (npred.masked_fill(~m, 1.0) * ngt.masked_fill(~m, 1.0)).sum(1, keepdim=True))
    return dot.masked_select(m).mean()


def grad_loss(gt, pred):
    loss = torch.zeros((), dtype=D, device=gt.device)
    g, p = gt.to(D), pred
    for lvl in range(4):
        if lvl:
            g, p = blur_pool2d(g), blur_pool2d(p)
        gg, gp = spatial_gradient(g), spatial_gradient(p)
        m = gg.isfinite()
        loss = loss + (gp.masked_select(m) - gg.masked_select(m)).abs().mean()
    return loss


def mv_project(depth, invK, wTc, K, cTw, eps=1e-8):
    """-> pixel x, pixel y, z' per pixel [B,h,w] (BackprojectDepth + Project3D)."""
    B, _, h, w = depth.shape
    cam = depth.flatten(2) * pix_rays(invK, h, w)
    world = wTc.to(D) @ torch.cat([cam, torch.ones_like(cam[:, :1])], 1)
    q = ((K.to(D) @ cTw.to(D))[:, :3]) @ world
    z = q[:, 2:] + eps
    sc = torch.where(q[:, 2:].abs() > eps, 1.0 / z, torch.ones_like(z))
    pix = q[:, :2] * sc
    return pix[:, 0].view(B, h, w), pix[:, 1].view(B, h, w), z[:, 0].view(B, h, w)


def mv_sample(src, px, py):
    """grid_sample(nearest, align_corners=False, zeros) through the normalise / unnormalise round trip."""
    B, h, w = px.shape
    ix = ((2.0 * (px / w) - 1.0 + 1.0) * w - 1.0) / 2.0
    iy = ((2.0 * (py / h) - 1.0 + 1.0) * h - 1.0) / 2.0
    rx, ry = torch.round(ix), torch.round(iy)   # half to even
    ok = (rx >= 0) & (rx <= w - 1) & (ry >= 0) & (ry <= h - 1)
    idx = (ry.clamp(0, h - 1) * w + rx.clamp(0, w - 1)).nan_to_num(0).long().view(B, -1)
    s = torch.gather(src.to(D).reshape(B, -1), 1, idx).view(B, h, w)
    return torch.where(ok, s, torch.zeros_like(s)), ix, iy


def mv_pair(pred, gt, src, invK, srcK, wTc, cTw):
    """-> (error terms [B,h,w] with NaN where not counted, valid mask, ambiguous mask, sampled depth)."""
    px, py, zq = mv_project(gt.to(D), invK, wTc, srcK, cTw)
    s, ix, iy = mv_sample(src[:, 0], px, py)
    valid = (zq < 1.05 * s) & (zq > 0) & (s > 0)
    _, _, zp = mv_project(pred, invK, wTc, srcK, cTw)
    err = (torch.log(s) - torch.log(zp)).abs()
    counted = valid & ~err.isnan()
    rel = 1e-5
    amb = ((zq - 1.05 * s).abs() <= rel * zq.abs()) | ((ix - ix.floor() - 0.5).abs() <= rel * (ix.abs() + 1)) | \
          ((iy - iy.floor() - 0.5).abs() <= rel * (iy.abs() + 1))
    amb = amb & s.isfinite() & zq.isfinite()
    return torch.where(counted, err, torch.full_like(err, float("nan"))), valid, amb, s


def mv_loss(pred, gt, src_bk1hw, invK, srcK_bk, wTc, cTw_bk):
    K = src_bk1hw.shape[1]
    total = torch.zeros((), dtype=D, device=pred.device)
    for k in range(K):
        e, _, _, _ = mv_pair(pred, gt, src_bk1hw[:, k], invK, srcK_bk[:, k], wTc, cTw_bk[:, k])
        total = total + e.nanmean()
    return total / K


def nearest(x, h, w):
    """F.interpolate(mode="nearest") indices in fp32, as ATen computes them."""
    def idx(out, inp):
        if out == inp:
            return torch.arange(out, device=x.device)
        if out == 2 * inp:
            return torch.arange(out, device=x.device) // 2
        sc = torch.tensor(inp / out, dtype=torch.float32, device=x.device)
        return torch.clamp(torch.floor(torch.arange(out, dtype=torch.float32, device=x.device) * sc).long(), max=inp - 1)
    return x[..., idx(h, x.shape[-2])[:, None], idx(w, x.shape[-1])[None, :]]


def compute_losses(cur_data, src_data, outputs):
    """The nine terms in fp64 (inputs are cast; predictions keep their autograd graph)."""
    gt = cur_data["depth_b1hw"].to(D)
    mask = cur_data["mask_b_b1hw"]
    pred = outputs["depth_pred_s0_b1hw"]
    log_pred = outputs["log_depth_pred_s0_b1hw"]
    # log of the fp32 gt rounded to fp32, as the reference takes it: a prediction equal to it is a tie (|.|' = 0)
    lgt = torch.log(cur_data["depth_b1hw"].float()).to(D)
    ms, found = 0, False
    for i in range(4):
        k = f"log_depth_pred_s{i}_b1hw"
        if k in outputs:
            r = nearest(outputs[k], *gt.shape[-2:])
            ms = ms + (lgt[mask] - r[mask]).abs().mean() / 2 ** i
            found = True
    if not found:
        raise Exception("Could not find a valid scale to compute si loss!")
    gl = grad_loss(gt, pred)
    absl = (gt[mask] - pred[mask]).abs().mean()
    d = lgt[mask] - log_pred[mask]
    si = torch.sqrt((d ** 2).mean() - 0.85 * d.mean() ** 2)
    m2 = mask & (pred > 0.1)
    inv = (1 / gt[m2] - 1 / pred[m2]).abs().mean()
    l1 = (lgt[mask] - log_pred[mask]).abs().mean()
    nl = normals_loss(cur_data["normals_b3hw"].to(D), outputs["normals_pred_b3hw"])
    mv = mv_loss(pred, gt, src_data["depth_b1hw"], cur_data["invK_s0_b44"], src_data["K_s0_b44"],
                 cur_data["world_T_cam_b44"], src_data["cam_T_world_b44"])
    return {"loss": ms + gl + nl + 0.2 * mv, "si_loss": si, "grad_loss": gl, "abs_loss": absl, "normals_loss": nl,
            "ms_loss": ms, "inv_abs_loss": inv, "log_l1_loss": l1, "mv_loss": mv}


def run(inputs, want_grads=True):
    """`inputs`: a dict of numpy / torch arrays as stored in tests/golden/loss_<case>.npz.  Returns the terms, both
    normal maps, the multi-view ambiguity masks and (optionally) the gradients of `loss` and of each term with respect
    to depth_pred and each log_depth_pred_s{i}, all as fp64 tensors.  Normals are computed from the fp64 depths and
    are leaves of the loss (as in the reference's step: the normals loss reaches depth_pred only through them)."""
    t = {k: torch.as_tensor(v) for k, v in inputs.items()}
    scales = [i for i in range(4) if f"log_depth_pred_s{i}_b1hw" in t]
    cur = {"depth_b1hw": t["depth_b1hw"], "mask_b_b1hw": t["mask_b_b1hw"].bool(), "invK_s0_b44": t["invK_s0_b44"],
           "world_T_cam_b44": t["world_T_cam_b44"]}
    src = {"depth_b1hw": t["src_depth_bk1hw"], "K_s0_b44": t["src_K_s0_bk44"], "cam_T_world_b44": t["src_cam_T_world_bk44"]}
    pred = t["depth_pred_s0_b1hw"].to(D).requires_grad_(True)
    logs = {i: t[f"log_depth_pred_s{i}_b1hw"].to(D).requires_grad_(True) for i in scales}
    ngt = normals(t["depth_b1hw"], t["invK_s0_b44"])
    npred = normals(pred, t["invK_s0_b44"])
    cur["normals_b3hw"] = ngt
    outputs = {"depth_pred_s0_b1hw": pred, "normals_pred_b3hw": npred}
    outputs.update({f"log_depth_pred_s{i}_b1hw": v for i, v in logs.items()})
    terms = compute_losses(cur, src, outputs)
    res = {"terms": {k: v.detach() for k, v in terms.items()}, "normals_gt": ngt.detach(), "normals_pred": npred.detach()}
    amb = []
    for k in range(t["src_depth_bk1hw"].shape[1]):
        _, valid, a, _ = mv_pair(pred.detach(), t["depth_b1hw"], t["src_depth_bk1hw"][:, k], t["invK_s0_b44"],
                                 t["src_K_s0_bk44"][:, k], t["world_T_cam_b44"], t["src_cam_T_world_bk44"][:, k])
        amb.append(a)
    res["mv_ambiguous"] = torch.stack(amb, 1)
    if want_grads:
        leaves = [pred] + [logs[i] for i in scales]
        names = ["depth_pred_s0_b1hw"] + [f"log_depth_pred_s{i}_b1hw" for i in scales]
        grads = {}
        for key in KEYS:
            v = terms[key]
            if not v.requires_grad:
                continue
            gs = torch.autograd.grad(v, leaves, retain_graph=True, allow_unused=True)
            for n, g in zip(names, gs):
                grads[f"{key}/{n}"] = torch.zeros_like(leaves[names.index(n)]) if g is None else g
        res["grads"] = grads
    return res


def rel_err(got, want):
    got, want = torch.as_tensor(got, dtype=D), torch.as_tensor(want, dtype=D)
    fin = want.isfinite()
    if not torch.equal(fin, got.isfinite()):
        return math.inf
    if not fin.any():
        return 0.0
    scale = want[fin].abs().max().clamp_min(1e-30)
    return float((got[fin] - want[fin]).abs().max() / scale)
