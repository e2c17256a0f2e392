"""The reference's training losses (losses.py; experiment_modules/depth_model.py:409-500), API-compatible, on the HIP
kernels of csrc/sr_losses.hip.  The rules are stated in include/simplerecon_hip.h, section "training losses".

Each loss is a torch.autograd.Function over one fused forward entry point and one backward entry point.  A forward
returns a small device vector (the loss and the counts / means its backward needs); torch only allocates, slices and
adds the final scalars.  Nothing here synchronises the host.  Gradients flow to the predictions only: gt depth,
masks, poses and intrinsics are data, and asking for their gradient raises.  Everything is fp32; under autocast the
losses still run in fp32 (the reference runs their matmuls in fp16 there)."""
import torch
from torch import nn

from . import _lib

MAX_SOURCES = 15   # SR_LOSS_MAX_SOURCES
PROJECT_EPS = 1e-8   # Project3D's eps


_FP32 = "the losses run in fp32"
_DATA = "it is data for the training losses"


def _dev(name, t, min_hw=3):
    t = _lib.device_f32(name, t, _FP32)
    if t.dim() < 2 or t.shape[-1] < min_hw or t.shape[-2] < min_hw:
        raise ValueError(f"{name} {tuple(t.shape)}: the losses need maps of at least {min_hw}x{min_hw}")
    return t


def _mask(name, t):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise _lib.HipLibraryError(f"{name} must be a device tensor (no CPU fallback)")
    if t.dtype != torch.bool:
        raise TypeError(f"{name} must be a bool mask, got {t.dtype}")
    return t.contiguous().view(torch.uint8)


def _ws(nbytes, device, what):
    if nbytes == 0:
        raise ValueError(f"{what}: shape refused by the library")
    return torch.empty(int(nbytes), dtype=torch.uint8, device=device)


# ------------------------------------------------------------------------------------------------ normals -----------
class _Normals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, invK):
        B, h, w = _lib.map_bhw("depth", depth)
        dev = depth.device
        ws = _ws(_lib.lib().sr_normals_workspace_bytes(B, h, w), dev, "normals")
        out = torch.empty((B, 3, h, w), dtype=torch.float32, device=dev)
        _lib.call("sr_normals_fwd", dev, depth, invK, B, h, w, out, ws, ws.numel())
        ctx.save_for_backward(depth, invK)
        return out

    @staticmethod
    def backward(ctx, g):
        depth, invK = ctx.saved_tensors
        B, h, w = _lib.map_bhw("depth", depth)
        dev = depth.device
        g = g.contiguous()
        ws = _ws(_lib.lib().sr_normals_workspace_bytes(B, h, w), dev, "normals")
        gd = torch.empty_like(depth)
        _lib.call("sr_normals_bwd", dev, g, depth, invK, B, h, w, gd, ws, ws.numel())
        return gd, None


def normals_from_depth(depth_b1hw, invK_b44):
    """NormalGenerator(h, w)(depth, invK) with the reference's 5x5 / std 2 blur: [B,3,h,w]."""
    depth = _dev("depth_b1hw", depth_b1hw)
    invK = _lib.data_f32("invK_b44", invK_b44, _DATA, _FP32)
    if tuple(invK.shape) != (depth.shape[0], 4, 4):
        raise ValueError("expected invK [B,4,4]")
    return _Normals.apply(depth, invK)


class _NormalsLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ngt, npred):
        B, _, h, w = npred.shape
        dev = npred.device
        ws = _ws(_lib.lib().sr_normals_loss_workspace_bytes(B, h, w), dev, "normals loss")
        out = torch.empty(2, dtype=torch.float32, device=dev)
        _lib.call("sr_normals_loss_fwd", dev, ngt, npred, B, h, w, out, ws, ws.numel())
        ctx.save_for_backward(ngt, npred, out)
        return out

    @staticmethod
    def backward(ctx, g):
        ngt, npred, stats = ctx.saved_tensors
        B, _, h, w = npred.shape
        g = g.contiguous()
        gp = torch.empty_like(npred)
        _lib.call("sr_normals_loss_bwd", npred.device, g, stats, ngt, npred, B, h, w, gp)
        return None, gp


class NormalsLoss(nn.Module):
    """Reference losses.py:57-77: the masked mean of 0.5 (1 - n_pred . n_gt) over the pixels where both are finite."""

    def forward(self, normals_gt_b3hw, normals_pred_b3hw):
        ngt = _lib.data_f32("normals_gt_b3hw", normals_gt_b3hw, _DATA, _FP32)
        npred = _dev("normals_pred_b3hw", normals_pred_b3hw)
        if npred.dim() != 4 or npred.shape[1] != 3 or ngt.shape != npred.shape:
            raise ValueError("expected normals [B,3,h,w] of equal shape")
        return _NormalsLoss.apply(ngt, npred)[0]


# -------------------------------------------------------------------------------------------- grad loss -------------
class _GradLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gt, pred):
        B, h, w = _lib.map_bhw("pred", pred)
        dev = pred.device
        ws = _ws(_lib.lib().sr_grad_loss_workspace_bytes(B, h, w), dev, "gradient loss")
        out = torch.empty(5, dtype=torch.float32, device=dev)
        _lib.call("sr_grad_loss_fwd", dev, gt, pred, B, h, w, out, ws, ws.numel())
        ctx.save_for_backward(gt, pred, out)
        ctx.ws = ws   # the backward reads the pyramid the forward left here
        return out

    @staticmethod
    def backward(ctx, g):
        gt, pred, stats = ctx.saved_tensors
        B, h, w = _lib.map_bhw("pred", pred)
        g = g.contiguous()
        gp = torch.empty_like(pred)
        ws = ctx.ws
        _lib.call("sr_grad_loss_bwd", pred.device, g, stats, gt, pred, B, h, w, gp, ws, ws.numel())
        return None, gp


class MSGradientLoss(nn.Module):
    """Reference losses.py:11-37: the sum over a 4-level blur-pool pyramid of the mean |grad pred - grad gt| over the
    gradient components whose gt value is finite."""

    def __init__(self, num_scales: int = 4):
        super().__init__()
        if num_scales != 4:
            raise ValueError("the HIP gradient loss implements the reference's 4-level pyramid only")
        self.num_scales = num_scales

    def forward(self, depth_gt, depth_pred):
        gt = _lib.data_f32("depth_gt", depth_gt, _DATA, _FP32)
        pred = _dev("depth_pred", depth_pred)
        if gt.shape != pred.shape:
            raise ValueError("depth_gt and depth_pred differ in shape")
        _lib.map_bhw("depth_pred", pred)
        return _GradLoss.apply(gt, pred)[0]


# ------------------------------------------------------------------------------------------- multi-view -------------
def _mv_args(cur_depth, src_depth, cur_invK, src_K, cur_world_T_cam, src_cam_T_world, height, width):
    gt = _lib.data_f32("cur_depth_b1hw", cur_depth, _DATA, _FP32)
    B, h, w = _lib.map_bhw("cur_depth_b1hw", gt)
    if (h, w) != (height, width) or h < 3 or w < 3:
        raise ValueError(f"depth {tuple(gt.shape)} does not match {height}x{width}")
    src = _lib.data_f32("src_depth", src_depth, _DATA, _FP32)
    K = src.shape[1] if src.dim() == 5 else 1
    if not 1 <= K <= MAX_SOURCES:
        raise ValueError(f"{K} source views: the multi-view loss takes 1..{MAX_SOURCES}")
    if src.numel() != B * K * h * w:
        raise ValueError("source depths do not match the current depth map")
    mats = [_lib.data_f32(n, m, _DATA, _FP32) for n, m in (("cur_invK_b44", cur_invK), ("src_K", src_K),
                                                           ("cur_world_T_cam_b44", cur_world_T_cam),
                                                           ("src_cam_T_world", src_cam_T_world))]
    for m, n in zip(mats, (B, B * K, B, B * K)):
        if m.numel() != n * 16:
            raise ValueError("expected [B,4,4] current and [B,K,4,4] source matrices")
    return gt, src, mats, B, K, h, w


class _MVLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, src, invK, srcK, wTc, cTw, K):
        B, h, w = _lib.map_bhw("pred", pred)
        dev = pred.device
        ws = _ws(_lib.lib().sr_mv_loss_workspace_bytes(B, K, h, w), dev, "multi-view loss")
        out = torch.empty(1 + 2 * K, dtype=torch.float32, device=dev)
        _lib.call("sr_mv_loss_fwd", dev, pred, gt, src, invK, srcK, wTc, cTw, B, K, h, w, PROJECT_EPS, out, None, None, ws,
                  ws.numel())
        ctx.save_for_backward(pred, gt, src, invK, srcK, wTc, cTw, out)
        ctx.K = K
        return out

    @staticmethod
    def backward(ctx, g):
        pred, gt, src, invK, srcK, wTc, cTw, stats = ctx.saved_tensors
        B, h, w = _lib.map_bhw("pred", pred)
        g = g.contiguous()
        gp = torch.empty_like(pred)
        _lib.call("sr_mv_loss_bwd", pred.device, g, stats, pred, gt, src, invK, srcK, wTc, cTw, B, ctx.K, h, w, PROJECT_EPS,
                  gp)
        return gp, None, None, None, None, None, None, None


class MVDepthLoss(nn.Module):
    """Reference losses.py:79-208.  All K sources run in one launch (a thread per pixel loops over them)."""

    def __init__(self, height, width):
        super().__init__()
        self.height, self.width = height, width

    def get_valid_mask(self, cur_depth_b1hw, src_depth_b1hw, cur_invK_b44, src_K_b44, cur_world_T_cam_b44,
                       src_cam_T_world_b44):
        """-> (valid_mask_b1hw bool, src_depth_sampled_b1hw) for one source view."""
        gt, src, (invK, srcK, wTc, cTw), B, K, h, w = _mv_args(cur_depth_b1hw, src_depth_b1hw, cur_invK_b44, src_K_b44,
                                                                cur_world_T_cam_b44, src_cam_T_world_b44,
                                                                self.height, self.width)
        dev = gt.device
        ws = _ws(_lib.lib().sr_mv_loss_workspace_bytes(B, K, h, w), dev, "multi-view loss")
        out = torch.empty(1 + 2 * K, dtype=torch.float32, device=dev)
        valid = torch.empty((B, K, h, w), dtype=torch.uint8, device=dev)
        sampled = torch.empty((B, K, h, w), dtype=torch.float32, device=dev)
        _lib.call("sr_mv_loss_fwd", dev, gt, gt, src, invK, srcK, wTc, cTw, B, K, h, w, PROJECT_EPS, out, valid, sampled, ws,
                  ws.numel())
        if K == 1:
            return valid.view(torch.bool), sampled
        return valid.view(torch.bool).view(B, K, 1, h, w), sampled.view(B, K, 1, h, w)

    def _loss(self, depth_pred_b1hw, cur_depth_b1hw, src_depth, cur_invK_b44, src_K, cur_world_T_cam_b44,
              src_cam_T_world):
        gt, src, (invK, srcK, wTc, cTw), B, K, h, w = _mv_args(cur_depth_b1hw, src_depth, cur_invK_b44, src_K,
                                                                cur_world_T_cam_b44, src_cam_T_world,
                                                                self.height, self.width)
        pred = _dev("depth_pred_b1hw", depth_pred_b1hw)
        if pred.shape != gt.shape:
            raise ValueError("depth_pred_b1hw and cur_depth_b1hw differ in shape")
        return _MVLoss.apply(pred, gt, src, invK, srcK, wTc, cTw, K)

    def get_error_for_pair(self, depth_pred_b1hw, cur_depth_b1hw, src_depth_b1hw, cur_invK_b44, src_K_b44,
                           cur_world_T_cam_b44, src_cam_T_world_b44):
        return self._loss(depth_pred_b1hw, cur_depth_b1hw, src_depth_b1hw, cur_invK_b44, src_K_b44,
                          cur_world_T_cam_b44, src_cam_T_world_b44)[0]

    def forward(self, depth_pred_b1hw, cur_depth_b1hw, src_depth_bk1hw, cur_invK_b44, src_K_bk44,
                cur_world_T_cam_b44, src_cam_T_world_bk44):
        if src_depth_bk1hw.dim() != 5:
            raise ValueError("expected source depths [B,K,1,h,w]")
        return self._loss(depth_pred_b1hw, cur_depth_b1hw, src_depth_bk1hw, cur_invK_b44, src_K_bk44,
                          cur_world_T_cam_b44, src_cam_T_world_bk44)[0]


# ------------------------------------------------------------------------------------------ depth terms -------------
DEPTH_TERMS = ("ms_loss", "abs_loss", "inv_abs_loss", "log_l1_loss", "si_loss")


class _DepthTerms(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gt, mask, pred, si_lambda, gt_is_log, l0, l1, l2, l3):
        B, h, w = _lib.map_bhw("gt", gt)
        dev = gt.device
        logs = [l0, l1, l2, l3]
        dims = []
        for t in logs[1:]:
            dims += [t, t.shape[-2] if t is not None else 0, t.shape[-1] if t is not None else 0]
        ws = _ws(_lib.lib().sr_depth_terms_workspace_bytes(B, h, w), dev, "depth terms")
        out = torch.empty(8, dtype=torch.float32, device=dev)
        _lib.call("sr_depth_terms_fwd", dev, gt, mask, pred, l0, *dims, B, h, w, si_lambda, int(gt_is_log), out, ws,
                  ws.numel())
        ctx.save_for_backward(gt, mask, pred, out, *[t if t is not None else torch.empty(0) for t in logs])
        ctx.present = [t is not None for t in logs]
        ctx.si_lambda, ctx.gt_is_log = si_lambda, gt_is_log
        return out

    @staticmethod
    def backward(ctx, g):
        gt, mask, pred, stats, *logs = ctx.saved_tensors
        logs = [t if p else None for t, p in zip(logs, ctx.present)]
        B, h, w = _lib.map_bhw("gt", gt)
        dev = gt.device
        g = g.contiguous()
        gpred = torch.empty_like(pred)
        glogs = [torch.empty_like(t) if t is not None else None for t in logs]
        dims = []
        for t in logs[1:]:
            dims += [t, t.shape[-2] if t is not None else 0, t.shape[-1] if t is not None else 0]
        _lib.call("sr_depth_terms_bwd", dev, g, stats, gt, mask, pred, logs[0], *dims, B, h, w, ctx.si_lambda,
                  int(ctx.gt_is_log), gpred, *glogs)
        return (None, None, gpred, None, None, *glogs)


def depth_terms(depth_gt, mask_b, depth_pred, log_depth_preds, si_lambda=0.85):
    """compute_losses' depth terms (reference depth_model.py:447-479) in one launch + finalize: a dict of the five
    scalars of DEPTH_TERMS.  `log_depth_preds`: {scale i: log_depth_pred_s{i}_b1hw}; scale 0 must be at gt size."""
    gt = _lib.data_f32("depth_b1hw", depth_gt, _DATA, _FP32)
    B, h, w = _lib.map_bhw("depth_b1hw", gt)
    mask = _mask("mask_b_b1hw", mask_b)
    pred = _dev("depth_pred_s0_b1hw", depth_pred, 1)
    if not log_depth_preds:
        raise ValueError("Could not find a valid scale to compute si loss!")
    if 0 not in log_depth_preds:
        raise KeyError("log_depth_pred_s0_b1hw")
    logs = [None] * 4
    for i, t in log_depth_preds.items():
        t = _dev(f"log_depth_pred_s{i}_b1hw", t, 1)
        if t.shape[0] != B or t.numel() != B * t.shape[-2] * t.shape[-1] or t.shape[-2] > h or t.shape[-1] > w:
            raise ValueError(f"log_depth_pred_s{i}_b1hw {tuple(t.shape)} does not fit the gt map {tuple(gt.shape)}")
        logs[i] = t
    if logs[0].shape[-2:] != gt.shape[-2:] or pred.shape != gt.shape or mask.numel() != gt.numel():
        raise ValueError("depth_pred_s0, log_depth_pred_s0 and the mask must match the gt map")
    out = _DepthTerms.apply(gt, mask, pred, float(si_lambda), False, *logs)
    return {k: out[i] for i, k in enumerate(DEPTH_TERMS)}


class ScaleInvariantLoss(nn.Module):
    """Reference losses.py:39-55 on tensors of any shape (typically the mask-selected log depths)."""

    def __init__(self, si_lambda: float = 0.85):
        super().__init__()
        self.si_lambda = si_lambda

    def forward(self, log_depth_gt, log_depth_pred):
        lgt = _lib.data_f32("log_depth_gt", log_depth_gt, _DATA, _FP32)
        _lib.device_f32("log_depth_pred", log_depth_pred, _FP32)
        if lgt.shape != log_depth_pred.shape or lgt.numel() == 0:
            raise ValueError("log_depth_gt and log_depth_pred must have the same, non-empty shape")
        n = lgt.numel()
        lp = log_depth_pred.contiguous().view(1, 1, n)
        mask = torch.ones((1, 1, n), dtype=torch.uint8, device=lgt.device)
        out = _DepthTerms.apply(lgt.view(1, 1, n), mask, lp, float(self.si_lambda), True, lp, None, None, None)
        return out[4]
