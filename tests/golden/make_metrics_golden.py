"""Writes tests/golden/metrics_<case>.npz and tests/golden/metrics_averager.json: what the reference's OWN
utils/metrics_utils.py computes on the CPU, driven as test.py (nearest upsample, gt > 0.5, the batched rule with
mult_a=True) and as the validation step (the pooled rule on a masked selection) do.  Needs a checkout of the reference;
pass its root.  metrics_utils.py imports only torch, numpy and json, so no shims are needed.

    python tests/golden/make_metrics_golden.py /path/to/simplerecon

npz fields: gt [B,H,W], pred [B,h,w], mode ("batched" | "pooled"), mask [B,H,W] (pooled), mult_a, n_valid [B]
(batched) and one array per metric key ([B] batched, scalar pooled)."""
import contextlib
import importlib.util
import io
import json
import os
import sys
import tempfile

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("abs_diff", "abs_rel", "sq_rel", "rmse", "rmse_log", "a5", "a10", "a25", "a0", "a1", "a2", "a3")
F32 = np.float32


def _up(a, b):
    return np.nextafter(F32(a), F32(b), dtype=F32)


def _depth(rng, B, h, w, lo=0.3, hi=6.0):
    return rng.uniform(lo, hi, size=(B, h, w)).astype(F32)


def cases():
    rng = np.random.default_rng(2024)
    out = {}
    # the quirk frame: pred < 0, pred == 0, NaN, exactly 1.05f, exact, inf
    gt = np.array([[[1, 2, 1, 1, 1, 1]]], F32)
    pred = np.array([[[-1, 0, np.nan, F32(1.05), 1, np.inf]]], F32)
    out["quirk"] = dict(gt=gt, pred=pred, mode="batched")
    out["quirk_pooled"] = dict(gt=gt, pred=pred, mode="pooled", mask=np.ones_like(gt, bool))
    # ratios exactly at each fp32 threshold and one ulp either side, both ways round
    ts = [1.05, 1.1, 1.25, 1.5625, 1.953125]
    r = []
    for t in ts:
        r += [F32(t), _up(t, 0), _up(t, 10)]
    r = np.array(r, F32)
    gt = np.concatenate([np.ones_like(r), r])[None, None]
    pred = np.concatenate([r, np.ones_like(r)])[None, None]
    out["thresholds"] = dict(gt=gt, pred=pred, mode="batched")
    # gt at, just above and just below 0.5
    g = np.array([0.5, _up(0.5, 1), _up(0.5, 0), 0.5, _up(0.5, 1), _up(0.5, 0), 0.7, 0.4], F32)
    p = np.array([0.5, 0.52, 0.48, 0.9, 0.45, 0.6, 0.75, 0.41], F32)
    out["min_depth"] = dict(gt=g[None, None], pred=p[None, None], mode="batched")
    # NaN and inf in gt and pred
    gt = _depth(rng, 2, 6, 8)
    pred = gt * rng.uniform(0.8, 1.25, size=gt.shape).astype(F32)
    gt[0, 0, :4] = [np.nan, np.inf, -np.inf, 0.0]
    pred[0, 1, :4] = [np.nan, np.inf, -np.inf, 0.0]
    gt[1, 2, 2], pred[1, 2, 2] = np.inf, np.inf
    gt[1, 3, 3], pred[1, 3, 3] = np.nan, np.nan
    pred[1, 4, :3] = [-np.inf, -2.0, np.nan]
    out["nonfinite"] = dict(gt=gt, pred=pred, mode="batched")
    # a frame without a valid pixel, between two ordinary ones
    gt = _depth(rng, 3, 8, 12)
    gt[1] = rng.uniform(0.0, 0.5, size=gt[1].shape).astype(F32)
    gt[1, :2] = np.nan
    pred = gt * rng.uniform(0.9, 1.1, size=gt.shape).astype(F32)
    pred[1] = 1.0
    out["empty_frame"] = dict(gt=gt, pred=pred, mode="batched")
    # nearest resampling: 1x, 2x, 2.5x, odd, downsample
    for name, (h, w, H, W) in {"nn_1x": (24, 32, 24, 32), "nn_2x": (24, 32, 48, 64), "nn_2p5x": (16, 20, 40, 50),
                               "nn_odd": (37, 53, 101, 149), "nn_down": (60, 80, 45, 70)}.items():
        gt = _depth(rng, 2, H, W)
        gt[:, ::7, ::5] = 0.0   # holes
        pred = _depth(rng, 2, h, w)
        out[name] = dict(gt=gt, pred=pred, mode="batched")
    # explicit masks, pooled rule (validation step): identity, a NaN term inside / outside the mask, an empty mask
    gt = _depth(rng, 2, 12, 16)
    pred = gt * rng.uniform(0.7, 1.3, size=gt.shape).astype(F32)
    mask = rng.uniform(size=gt.shape) < 0.6
    out["pooled_mask"] = dict(gt=gt, pred=pred, mode="pooled", mask=mask)
    gt2, pred2 = gt.copy(), pred.copy()
    pred2[0, 0, 0], mask2 = -1.0, mask.copy()
    mask2[0, 0, 0] = True     # log term NaN inside the mask: rmse_log is NaN
    pred2[1, 5, 5], mask2[1, 5, 5] = np.nan, False   # NaN outside the mask: no effect
    out["pooled_nan"] = dict(gt=gt2, pred=pred2, mode="pooled", mask=mask2)
    out["pooled_empty"] = dict(gt=gt, pred=pred, mode="pooled", mask=np.zeros_like(mask))
    # nearest-upsampled prediction under a mask, pooled
    gt = _depth(rng, 2, 30, 40)
    out["pooled_nn"] = dict(gt=gt, pred=_depth(rng, 2, 12, 16), mode="pooled", mask=rng.uniform(size=gt.shape) < 0.5)
    return out


def run_reference(mu, case):
    gt = torch.from_numpy(case["gt"])
    pred = torch.from_numpy(case["pred"])
    H, W = gt.shape[-2:]
    up = F.interpolate(pred.unsqueeze(1), size=(H, W), mode="nearest").squeeze(1)
    res = {}
    if case["mode"] == "batched":
        valid = gt > 0.5
        m = mu.compute_depth_metrics_batched(gt.flatten(start_dim=1).float(), up.flatten(start_dim=1).float(),
                                             valid.flatten(start_dim=1), mult_a=True)
        res["n_valid"] = valid.flatten(start_dim=1).sum(1).numpy().astype(np.int64)
        res["mult_a"] = np.array(True)
    else:
        mask = torch.from_numpy(case["mask"])
        m = mu.compute_depth_metrics(gt[mask], up[mask])
        res["mult_a"] = np.array(False)
    assert list(m) == list(KEYS)
    for k in KEYS:
        res[k] = m[k].numpy().astype(F32)
    return res


def averager_golden(mu):
    """The reference's ResultsAverager driven as test.py drives it, on fixed per-frame values: stdout and file bytes."""
    rng = np.random.default_rng(77)
    scenes = []
    for s, n in (("scene0000_00", 3), ("scan/0001", 4), ("scene0002_01", 1)):
        frames = []
        for _ in range(n):
            v = {k: float(F32(rng.uniform(0.01, 0.5) if k[0] != "a" else rng.uniform(60.0, 100.0))) for k in KEYS}
            v["model_time"] = float(rng.uniform(2.0, 40.0)) / 8
            frames.append(v)
        scenes.append((s, frames))
    buf = io.StringIO()
    files = {}
    with tempfile.TemporaryDirectory() as d, contextlib.redirect_stdout(buf):
        all_frame = mu.ResultsAverager("exp", "frame metrics")
        all_scene = mu.ResultsAverager("exp", "scene metrics")
        for scan, frames in scenes:
            scene = mu.ResultsAverager("exp", f"scene {scan} metrics")
            for v in frames:
                e = {k: (torch.tensor(x, dtype=torch.float32) if k != "model_time" else x) for k, x in v.items()}
                scene.update_results(e)
                all_frame.update_results(e)
            scene.compute_final_average()
            all_scene.update_results(scene.final_metrics)
            print("\nScene metrics:")
            scene.print_sheets_friendly(include_metrics_names=True)
            scene.output_json(os.path.join(d, f"{scan.replace('/', '_')}_metrics.json"))
            print("\nRunning frame metrics:")
            all_frame.print_sheets_friendly(include_metrics_names=False, print_running_metrics=True)
        print("\nFinal metrics:")
        all_scene.compute_final_average()
        all_scene.pretty_print_results(print_running_metrics=False)
        all_scene.print_sheets_friendly(include_metrics_names=True, print_running_metrics=False)
        all_scene.output_json(os.path.join(d, "all_scene_avg_metrics_test.json"))
        print("")
        all_frame.compute_final_average()
        all_frame.pretty_print_results(print_running_metrics=False)
        all_frame.print_sheets_friendly(include_metrics_names=True, print_running_metrics=False)
        all_frame.output_json(os.path.join(d, "all_frame_avg_metrics_test.json"))
        all_frame.compute_final_average(ignore_nans=True)
        all_frame.pretty_print_results(print_exp_name=False, print_running_metrics=True)
        empty = mu.ResultsAverager("exp", "empty")
        empty.compute_final_average()
        empty.print_sheets_friendly()
        empty.pretty_print_results()
        empty.output_json(os.path.join(d, "empty.json"))
        for f in sorted(os.listdir(d)):
            with open(os.path.join(d, f)) as fh:
                files[f] = fh.read()
    return {"scenes": scenes, "stdout": buf.getvalue(), "files": files}


def main(ref_root):
    spec = importlib.util.spec_from_file_location("ref_metrics_utils", os.path.join(ref_root, "utils", "metrics_utils.py"))
    mu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mu)
    for name, case in cases().items():
        res = run_reference(mu, case)
        arrays = dict(gt=case["gt"], pred=case["pred"], mode=np.array(case["mode"]))
        if "mask" in case:
            arrays["mask"] = case["mask"]
        arrays.update(res)
        path = os.path.join(HERE, f"metrics_{name}.npz")
        np.savez_compressed(path, **arrays)
        print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    path = os.path.join(HERE, "metrics_averager.json")
    with open(path, "w") as f:
        json.dump(averager_golden(mu), f, indent=1)
    print(f"wrote {path}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
