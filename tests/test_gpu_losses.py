"""The HIP training losses (csrc/sr_losses.hip via simplerecon_amd.losses and DepthModel.compute_losses) against the
reference's own outputs (tests/golden/loss_<case>.npz) and the fp64 oracle (tests/loss_oracle.py): every term, both
normal maps and every gradient, plus the multi-view mask, the Sobel NaN rule, determinism, autocast, no host
synchronisation and the B=8, K=7, 240x320 shape.

Bars (largest error relative to the largest magnitude of the compared map): terms, normal maps and gradients 1e-4,
gradients of mv_loss / loss 5e-4 (the fp32 reference's own cancellation, tests/test_loss_oracle_golden.py).  All cases
passed these bars on an MI355X; the individual errors were not logged."""
import os
import types

import numpy as np
import pytest
import torch

import loss_cases
import loss_oracle as lo
from simplerecon_amd import losses
from simplerecon_amd.depth_model import DepthModel

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL, TOL_MV_GRAD = 1e-4, 5e-4
DEV = "cuda"


def _holder():
    h = types.SimpleNamespace(_loss_modules={})
    h._losses_for = types.MethodType(DepthModel._losses_for, h)
    return h


def hip_losses(inputs, holder=None):
    """-> (terms dict, normals gt, normals pred, leaves dict) through DepthModel.compute_losses / compute_normals."""
    holder = holder or _holder()
    t = {k: torch.as_tensor(v).to(DEV) for k, v in inputs.items()}
    pred = t["depth_pred_s0_b1hw"].clone().requires_grad_(True)
    leaves = {"depth_pred_s0_b1hw": pred}
    for i in range(4):
        k = f"log_depth_pred_s{i}_b1hw"
        if k in t:
            leaves[k] = t[k].clone().requires_grad_(True)
    cur = {"depth_b1hw": t["depth_b1hw"], "mask_b_b1hw": t["mask_b_b1hw"].bool(), "invK_s0_b44": t["invK_s0_b44"],
           "world_T_cam_b44": t["world_T_cam_b44"]}
    src = {"depth_b1hw": t["src_depth_bk1hw"], "K_s0_b44": t["src_K_s0_bk44"], "cam_T_world_b44": t["src_cam_T_world_bk44"]}
    cur["normals_b3hw"] = DepthModel.compute_normals(holder, t["depth_b1hw"], t["invK_s0_b44"])
    outputs = dict(leaves)
    outputs["normals_pred_b3hw"] = DepthModel.compute_normals(holder, pred, t["invK_s0_b44"])
    terms = DepthModel.compute_losses(holder, cur, src, outputs)
    return terms, cur["normals_b3hw"], outputs["normals_pred_b3hw"], leaves


def load(name):
    g = np.load(os.path.join(GOLDEN, f"loss_{name}.npz"))
    return g, {k: g[k] for k in g.files if not k.startswith(("term/", "grad/", "normals_"))}


def masked_err(got, want, keep):
    got, want = torch.as_tensor(got).double().cpu(), torch.as_tensor(want).double().cpu()
    keep = torch.as_tensor(keep).cpu().expand_as(want)
    return lo.rel_err(torch.where(keep, got, want), want)


@pytest.mark.gpu
@pytest.mark.parametrize("name", loss_cases.CASES)
def test_terms_normals_and_gradients_match_golden_and_oracle(name):
    g, inputs = load(name)
    orc = lo.run(inputs)
    terms, ngt, npred, leaves = hip_losses(inputs)
    assert set(terms) == set(lo.KEYS)
    for k in lo.KEYS:
        got = terms[k].detach().cpu()
        assert lo.rel_err(got, g[f"term/{k}"]) < TOL, (name, k, float(got), float(g[f"term/{k}"]))
        assert lo.rel_err(got, orc["terms"][k]) < TOL, (name, k)
    assert lo.rel_err(ngt.cpu(), g["normals_gt"]) < TOL and lo.rel_err(npred.detach().cpu(), g["normals_pred"]) < TOL
    # pixels whose multi-view decision is within rounding distance of a threshold, and log-depth ties (a prediction equal
    # to log gt up to an ulp of logf), are left out of the gradient comparison
    amb = orc["mv_ambiguous"].any(1, keepdim=True)
    lgt = torch.log(torch.as_tensor(inputs["depth_b1hw"]))
    for key in lo.KEYS:
        if not terms[key].requires_grad:
            continue
        names = list(leaves)
        gs = torch.autograd.grad(terms[key], [leaves[n] for n in names], retain_graph=True, allow_unused=True)
        for n, gr in zip(names, gs):
            want = g[f"grad/{key}/{n}"]
            gr = torch.zeros_like(leaves[n]) if gr is None else gr
            keep = torch.ones(want.shape, dtype=torch.bool)
            if n == "depth_pred_s0_b1hw":
                keep = ~amb
            elif n == "log_depth_pred_s0_b1hw":
                keep = ~((lgt - torch.as_tensor(inputs[n])).abs() <= 1e-6 * lgt.abs())
            tol = TOL_MV_GRAD if key in ("mv_loss", "loss") else TOL
            assert masked_err(gr, want, keep) < tol, (name, key, n, masked_err(gr, want, keep))
            assert masked_err(gr, orc["grads"][f"{key}/{n}"], keep) < tol, (name, key, n)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["holes", "room7", "behind"])
def test_multi_view_valid_mask_outside_the_ambiguous_band(name):
    _, inputs = load(name)
    t = {k: torch.as_tensor(v) for k, v in inputs.items()}
    B, K = t["src_depth_bk1hw"].shape[:2]
    h, w = t["depth_b1hw"].shape[-2:]
    mv = losses.MVDepthLoss(h, w)
    valid, sampled = mv.get_valid_mask(t["depth_b1hw"].to(DEV), t["src_depth_bk1hw"].to(DEV), t["invK_s0_b44"].to(DEV),
                                       t["src_K_s0_bk44"].to(DEV), t["world_T_cam_b44"].to(DEV),
                                       t["src_cam_T_world_bk44"].to(DEV))
    assert valid.shape == (B, K, 1, h, w) and valid.dtype == torch.bool
    for k in range(K):
        _, v_o, amb, s_o = lo.mv_pair(t["depth_pred_s0_b1hw"].double(), t["depth_b1hw"], t["src_depth_bk1hw"][:, k],
                                      t["invK_s0_b44"], t["src_K_s0_bk44"][:, k], t["world_T_cam_b44"],
                                      t["src_cam_T_world_bk44"][:, k])
        got = valid[:, k, 0].cpu()
        assert torch.equal(got[~amb], v_o[~amb]), (name, k, int((got != v_o)[~amb].sum()))
        assert v_o.any()
        # the one-source call agrees with the K-source call
        v1, s1 = mv.get_valid_mask(t["depth_b1hw"].to(DEV), t["src_depth_bk1hw"][:, k].to(DEV), t["invK_s0_b44"].to(DEV),
                                   t["src_K_s0_bk44"][:, k].to(DEV), t["world_T_cam_b44"].to(DEV),
                                   t["src_cam_T_world_bk44"][:, k].to(DEV))
        assert torch.equal(v1.cpu()[:, 0], got)
        assert torch.equal(s1.cpu().nan_to_num(-1.0), sampled[:, k].cpu().nan_to_num(-1.0))


@pytest.mark.gpu
def test_sobel_nan_rule_reaches_nine_components():
    """One NaN depth pixel makes nine x and nine y gradient components non-finite, zero-weight taps included: the
    gradient loss then counts 18 components fewer at level 0."""
    h, w = 16, 20
    gt = torch.rand((1, 1, h, w), generator=torch.Generator().manual_seed(0)) + 1.0
    pred = (gt * 1.1).to(DEV)
    gt_nan = gt.clone()
    gt_nan[0, 0, 7, 9] = float("nan")
    counts = []
    for g in (gt, gt_nan):
        out = losses._GradLoss.apply(g.to(DEV), pred)
        counts.append(out[1:].cpu())
    assert float(counts[0][0]) == 2 * h * w and float(counts[0][0] - counts[1][0]) == 18
    assert float(lo.spatial_gradient(gt_nan.double()).isfinite().logical_not().sum()) == 18


def _batch(B, K, h, w, seed=0):
    from simplerecon_amd import synthetic
    cur, src = synthetic.training_batch(B, K, h, w, seed=seed, device=DEV)
    g = torch.Generator().manual_seed(seed)
    gt = cur["depth_b1hw"]
    fill = torch.nan_to_num(gt, nan=2.0)
    log0 = (torch.log(fill).cpu() + 0.05 * torch.randn(gt.shape, generator=g)).to(DEV)
    outs = {"log_depth_pred_s0_b1hw": log0.requires_grad_(True)}
    x = log0.detach()
    for i in range(1, 4):
        x = torch.nn.functional.avg_pool2d(x, 2, ceil_mode=True)
        outs[f"log_depth_pred_s{i}_b1hw"] = x.clone().requires_grad_(True)
    outs["depth_pred_s0_b1hw"] = torch.exp(log0.detach()).requires_grad_(True)
    return cur, src, outs


def _run(holder, cur, src, outs):
    cur = dict(cur)
    o = dict(outs)
    cur["normals_b3hw"] = DepthModel.compute_normals(holder, cur["depth_b1hw"], cur["invK_s0_b44"])
    o["normals_pred_b3hw"] = DepthModel.compute_normals(holder, o["depth_pred_s0_b1hw"], cur["invK_s0_b44"])
    terms = DepthModel.compute_losses(holder, cur, src, o)
    leaves = [v for k, v in outs.items()]
    grads = torch.autograd.grad(terms["loss"], leaves)
    return torch.stack([terms[k].detach() for k in lo.KEYS]), grads


@pytest.mark.gpu
def test_run_to_run_bit_equal_autocast_identical_and_no_sync():
    holder = _holder()
    cur, src, outs = _batch(2, 3, 48, 64)
    t1, g1 = _run(holder, cur, src, outs)
    t2, g2 = _run(holder, cur, src, outs)
    assert torch.equal(t1, t2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    with torch.autocast("cuda", dtype=torch.float16):
        t3, g3 = _run(holder, cur, src, outs)
    assert torch.equal(t1, t3) and all(torch.equal(a, b) for a, b in zip(g1, g3))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        t4, g4 = _run(holder, cur, src, outs)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.equal(t1, t4) and all(torch.equal(a, b) for a, b in zip(g1, g4))


@pytest.mark.gpu
def test_full_shape_b8_k7_240x320_against_oracle():
    holder = _holder()
    cur, src, outs = _batch(8, 7, 240, 320, seed=3)
    terms, grads = _run(holder, cur, src, outs)
    inputs = {"depth_b1hw": cur["depth_b1hw"].cpu(), "mask_b_b1hw": cur["mask_b_b1hw"].cpu(),
              "invK_s0_b44": cur["invK_s0_b44"].cpu(), "world_T_cam_b44": cur["world_T_cam_b44"].cpu(),
              "src_depth_bk1hw": src["depth_b1hw"].cpu(), "src_K_s0_bk44": src["K_s0_b44"].cpu(),
              "src_cam_T_world_bk44": src["cam_T_world_b44"].cpu()}
    inputs.update({k: v.detach().cpu() for k, v in outs.items()})
    orc = lo.run(inputs, want_grads=False)
    for i, k in enumerate(lo.KEYS):
        assert lo.rel_err(terms[i].cpu(), orc["terms"][k]) < TOL, (k, float(terms[i]), float(orc["terms"][k]))
    assert all(bool(g.isfinite().all()) for g in grads)
