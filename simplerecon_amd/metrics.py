"""The reference's depth metrics (utils/metrics_utils.py), API-compatible, on the HIP kernels of csrc/sr_metrics.hip.
The rules, quirks included, are stated in include/simplerecon_hip.h, section "depth metrics".

    score_frames(gt_b1HW, pred_b1hw)            fused test-time scoring (test.py:263-303): [B] metrics + valid counts
    compute_depth_metrics_batched(gt, pred, m)  the reference's per-frame rule on [B,N] maps
    compute_depth_metrics(gt, pred)             the reference's pooled rule (validation step)
    ResultsAverager                             frame / scene averages and the JSON score files

Each call is two kernel launches and returns device tensors: nothing here synchronises the host except
ResultsAverager, which works on host values as the reference's does.  Inputs are fp32 device tensors; host tensors
and other dtypes are refused (no CPU fallback)."""
import json

import numpy as np
import torch

from . import _lib

METRIC_KEYS = ("abs_diff", "abs_rel", "sq_rel", "rmse", "rmse_log", "a5", "a10", "a25", "a0", "a1", "a2", "a3")
RESAMPLE_IDENTITY, RESAMPLE_NEAREST = 0, 1   # SR_RESAMPLE_*
MAX_PIXELS = 1 << 24                          # SR_METRICS_MAX_PIXELS


_FP32 = "the metrics run in fp32"


def _mask(name, t, like):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t)}")
    if not t.is_cuda:
        raise _lib.HipLibraryError(f"{name} lives on {t.device}: the HIP path needs device tensors (no CPU fallback)")
    if t.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"{name} must be a bool or uint8 mask, got {t.dtype}")
    if t.numel() != like.numel():
        raise ValueError(f"{name} {tuple(t.shape)} does not cover the ground truth {tuple(like.shape)}")
    return t.detach().contiguous().view(torch.uint8)


def _run(gt, pred, mask, min_depth, B, H, W, h, w, resample, mult_a, pooled):
    """-> one flat fp32 device buffer: [B*12] metrics, [B] int32 valid counts (as raw bits), then [12] pooled metrics
    when `pooled`.  One copy of it brings everything to the host; split_block() takes it apart."""
    dev = gt.device
    if pred.device != dev or (mask is not None and mask.device != dev):
        raise ValueError("gt, pred and mask must be on the same device")
    nbytes = _lib.lib().sr_depth_metrics_workspace_bytes(B, H, W)
    if nbytes == 0 or H * W > MAX_PIXELS or h * w > MAX_PIXELS:
        raise ValueError(f"depth metrics: shape B={B} {H}x{W} (pred {h}x{w}) refused by the library")
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    buf = torch.empty(B * 13 + (12 if pooled else 0), dtype=torch.float32, device=dev)
    block, counts = split_block(buf, B)
    _lib.call("sr_depth_metrics", dev, gt, pred, mask, float(min_depth), B, H, W, h, w,
              resample, 1 if mult_a else 0, block, counts, buf[B * 13:] if pooled else None, ws, ws.numel())
    return buf


def split_block(buf, B):
    """The buffer of score_block() (on the device or copied to the host) -> (metrics [B,12] fp32 in METRIC_KEYS order,
    valid counts [B] int32)."""
    return buf[:B * 12].view(B, 12), buf[B * 12:B * 13].view(torch.int32)


def _nan_metrics(device):
    return _as_dict(torch.full((12,), float("nan"), dtype=torch.float32, device=device))


def _as_dict(values):
    """[..., 12] -> the reference's dict, in its key order."""
    return {k: values[..., i] for i, k in enumerate(METRIC_KEYS)}


def score_block(depth_gt_b1HW, depth_pred_b1hw, min_depth=0.5, mask_b1HW=None, mult_a=True):
    """score_frames() as one flat device buffer of B*13 fp32 words (split_block() takes it apart), so that a single
    device-to-host copy brings the metrics and the valid counts of a batch to the host."""
    gt = _lib.device_f32("depth_gt_b1HW", depth_gt_b1HW, _FP32).detach()
    pred = _lib.device_f32("depth_pred_b1hw", depth_pred_b1hw, _FP32).detach()
    B, H, W = _lib.map_bhw("depth_gt_b1HW", gt)
    Bp, h, w = _lib.map_bhw("depth_pred_b1hw", pred)
    if Bp != B:
        raise ValueError(f"batch sizes differ: gt {B}, pred {Bp}")
    mask = None if mask_b1HW is None else _mask("mask_b1HW", mask_b1HW, gt)
    resample = RESAMPLE_IDENTITY if (h, w) == (H, W) else RESAMPLE_NEAREST
    return _run(gt, pred, mask, min_depth, B, H, W, h, w, resample, mult_a, False)


def score_frames(depth_gt_b1HW, depth_pred_b1hw, min_depth=0.5, mask_b1HW=None, mult_a=True):
    """The scoring of test.py:263-303 fused: the prediction is read through F.interpolate(mode="nearest") to the gt's
    size, valid = gt > min_depth (or `mask_b1HW` when given), compute_depth_metrics_batched(..., mult_a) per frame.

    Returns (dict of [B] fp32 tensors in the reference's key order, valid pixel count [B] int32).  A frame with count 0
    has NaN metrics; test.py skips it.  No host synchronisation."""
    buf = score_block(depth_gt_b1HW, depth_pred_b1hw, min_depth, mask_b1HW, mult_a)
    block, counts = split_block(buf, depth_gt_b1HW.shape[0])
    return _as_dict(block), counts


def compute_depth_metrics_batched(gt_bN, pred_bN, valid_masks_bN, mult_a=False):
    """The reference's batched rule (metrics_utils.py compute_depth_metrics_batched) on [B,N] maps: a dict of [B]
    tensors.  Invalid pixels are dropped, each error metric is a nanmean, the a-metrics divide by the valid count."""
    gt = _lib.device_f32("gt_bN", gt_bN, _FP32).detach()
    pred = _lib.device_f32("pred_bN", pred_bN, _FP32).detach()
    if gt.dim() != 2 or pred.shape != gt.shape:
        raise ValueError(f"expected gt_bN and pred_bN of one [B,N] shape, got {tuple(gt.shape)}, {tuple(pred.shape)}")
    mask = _mask("valid_masks_bN", valid_masks_bN, gt)
    B, N = gt.shape
    return _as_dict(split_block(_run(gt, pred, mask, 0.0, B, 1, N, 1, N, RESAMPLE_IDENTITY, mult_a, False), B)[0])


def masked_depth_metrics(gt, pred, mask, mult_a=False):
    """compute_depth_metrics(gt[mask], pred[mask], mult_a) without materialising the selection: gt, pred and mask of
    one shape; a dict of 0-dim tensors."""
    gt = _lib.device_f32("gt", gt, _FP32).detach()
    pred = _lib.device_f32("pred", pred, _FP32).detach()
    if pred.shape != gt.shape:
        raise ValueError(f"gt {tuple(gt.shape)} and pred {tuple(pred.shape)} differ")
    mask = _mask("mask", mask, gt)
    if gt.numel() == 0:
        return _nan_metrics(gt.device)   # the mean of an empty selection
    B = gt.shape[0] if gt.dim() >= 2 else 1
    N = gt.numel() // B
    return _as_dict(_run(gt, pred, mask, 0.0, B, 1, N, 1, N, RESAMPLE_IDENTITY, mult_a, True)[B * 13:])


def compute_depth_metrics(gt, pred, mult_a=False):
    """The reference's pooled rule (metrics_utils.py compute_depth_metrics) over every element of gt / pred (the
    reference calls it on masked selections): plain means, so a NaN term makes its metric NaN.  A dict of 0-dim
    tensors."""
    gt = _lib.device_f32("gt", gt, _FP32).detach()
    ones = torch.ones(gt.shape, dtype=torch.uint8, device=gt.device)
    return masked_depth_metrics(gt, pred, ones, mult_a)


# ------------------------------------------------------------------------------------------- averaging ------------
def _fmt(v):
    return f"{v:.4f},"


class ResultsAverager:
    """Frame and scene averages of metric dicts (the reference's metrics_utils.ResultsAverager: same methods, arguments,
    printed lines and JSON files).

    Two averages are kept: a running one, updated per element as (avg * n + x) / (n + 1) in the elements' own
    precision (fp32 for the per-frame metrics), and the final one, a numpy mean over every element, computed by
    compute_final_average()."""

    def __init__(self, exp_name, metrics_name):
        self.exp_name = exp_name
        self.metrics_name = metrics_name
        self.elem_metrics_list = []
        self.running_metrics = None
        self.running_count = 0
        self.final_computed_average = None

    def update_results(self, elem_metrics):
        self.elem_metrics_list.append(dict(elem_metrics))
        if self.running_metrics is None:
            self.running_metrics = dict(elem_metrics)
        else:
            n = self.running_count
            for key, value in elem_metrics.items():
                self.running_metrics[key] = (self.running_metrics[key] * n + value) / (n + 1)
        self.running_count += 1

    def _chosen(self, running):
        return self.running_metrics if running else self.final_metrics

    @staticmethod
    def _rows(metrics):
        names = "".join(f"{k:8} " for k in metrics)
        values = "".join(f"{_fmt(v):8} " for v in metrics.values())
        return names, values

    def print_sheets_friendly(self, print_exp_name=True, include_metrics_names=False, print_running_metrics=True):
        """One row of values (and optionally one of names), for pasting into a spreadsheet."""
        if print_exp_name:
            print(f"{self.exp_name}, {self.metrics_name}")
        metrics = self._chosen(print_running_metrics)
        if not self.elem_metrics_list:
            print("WARNING: No valid metrics to print.")
            return
        names, values = self._rows(metrics)
        if include_metrics_names:
            print(names)
        print(values)

    def output_json(self, filepath, print_running_metrics=False):
        """Writes exp_name, metrics_type, scores, metrics_string and scores_string to `filepath` (indent 4)."""
        metrics = self._chosen(print_running_metrics)
        if not self.elem_metrics_list:
            print("WARNING: No valid metrics will be output.")
        names, values = self._rows(metrics)
        out = {"exp_name": self.exp_name, "metrics_type": self.metrics_name,
               "scores": {k: float(v) for k, v in metrics.items()},
               "metrics_string": names, "scores_string": values}
        with open(filepath, "w") as f:
            json.dump(out, f, indent=4)

    def pretty_print_results(self, print_exp_name=True, print_running_metrics=True):
        """One `name: value` line per metric."""
        metrics = self._chosen(print_running_metrics)
        if not self.elem_metrics_list:
            print("WARNING: No valid metrics to print.")
            return
        if print_exp_name:
            print(f"{self.exp_name}, {self.metrics_name}")
        for k, v in metrics.items():
            print(f"{k:8}: {v:.4f}")

    def compute_final_average(self, ignore_nans=False):
        """final_metrics[key] = numpy mean (nanmean with ignore_nans) of the key's values over every element."""
        self.final_metrics = {}
        if not self.elem_metrics_list:
            print("WARNING: no valid entry to average!")
            return
        for key in self.running_metrics:
            values = np.array([e[key].cpu().numpy() if torch.is_tensor(e[key]) else e[key]
                               for e in self.elem_metrics_list])
            self.final_metrics[key] = np.nanmean(values) if ignore_nans else values.mean()


def _gather(pred_b1hw, H, W):
    """Tests only: the prediction read through the kernels' nearest index map at H x W ([B,H,W]), i.e. what
    F.interpolate(mode="nearest") gives."""
    pred = _lib.device_f32("pred_b1hw", pred_b1hw, _FP32).detach()
    B, h, w = _lib.map_bhw("pred_b1hw", pred)
    out = torch.empty((B, H, W), dtype=torch.float32, device=pred.device)
    _lib.call("sr_depth_metrics_gather", pred.device, pred, B, H, W, h, w, RESAMPLE_NEAREST, out)
    return out
