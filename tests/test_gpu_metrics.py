"""The HIP depth metrics (csrc/sr_metrics.hip via simplerecon_amd.metrics, DepthModel.compute_metrics and
evaluation.evaluate) against the reference's own outputs (tests/golden/metrics_<case>.npz) and the numpy oracle
(tests/metrics_oracle.py): exact counts and NaN / inf positions, values, the nearest index map, determinism across
runs and batch sizes, no host synchronisation, the pooled validation path and the scoring loop end to end."""
import json
import os
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import metrics_oracle as mo
from test_metrics_host import CASES, assert_metrics_match, load
from simplerecon_amd import depth_model as dm
from simplerecon_amd import metrics, synthetic
from simplerecon_amd.evaluation import evaluate

DEV = "cuda"
IDENTITY_CASES = ("quirk", "thresholds", "min_depth", "nonfinite", "empty_frame", "nn_1x")


def _host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def _scan_maps(B=8, H=480, W=640, h=192, w=256, seed=3):
    """Ray-cast gt at H x W with holes and a noisy ray-cast prediction at h x w (holes = 0 depth)."""
    gt = synthetic.raycast_scene(B, H, W, seed=seed, holes=0.02)["depths"]
    pred = synthetic.raycast_scene(B, h, w, seed=seed, noise=0.05, holes=0.01)["depths"]
    return gt.float().contiguous(), pred.float().contiguous()


def _close(got, want, rtol=1e-6, rtol_log=1e-5):
    for k in mo.KEYS:
        a, b = np.asarray(got[k], np.float64), np.asarray(want[k], np.float64)
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=k)
        fin = np.isfinite(b)
        np.testing.assert_allclose(a[fin], b[fin], rtol=rtol_log if k == "rmse_log" else rtol, atol=0, err_msg=k)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_metrics_match_reference_goldens(case):
    g = load(case)
    gt, pred = torch.from_numpy(g["gt"]).to(DEV), torch.from_numpy(g["pred"]).to(DEV)
    if str(g["mode"]) == "batched":
        m, n = metrics.score_frames(gt.unsqueeze(1), pred.unsqueeze(1))
        np.testing.assert_array_equal(n.cpu().numpy(), g["n_valid"])
        assert_metrics_match(_host(m), g)
        if case in IDENTITY_CASES:
            mb = metrics.compute_depth_metrics_batched(gt.flatten(1), pred.flatten(1), (gt > 0.5).flatten(1), mult_a=True)
            assert_metrics_match(_host(mb), g)
    else:
        mask = torch.from_numpy(g["mask"]).to(DEV)
        up = F.interpolate(pred.unsqueeze(1), size=gt.shape[-2:], mode="nearest").squeeze(1)
        assert_metrics_match(_host(metrics.compute_depth_metrics(gt[mask], up[mask])), g)
        assert_metrics_match(_host(metrics.masked_depth_metrics(gt, up, mask)), g)


@pytest.mark.gpu
def test_scoring_matches_oracle_at_scannet_shape():
    gt, pred = _scan_maps()
    m, n = metrics.score_frames(gt.to(DEV).unsqueeze(1), pred.to(DEV).unsqueeze(1))
    want, n_want = mo.score(gt.numpy(), pred.numpy())
    np.testing.assert_array_equal(n.cpu().numpy(), n_want)
    _close(_host(m), want)
    # explicit mask, and the pooled rule over the batch
    mask = (gt > 1.0).to(DEV)
    m2, n2 = metrics.score_frames(gt.to(DEV), pred.to(DEV), mask_b1HW=mask, mult_a=False)
    up = mo.upsample_nearest(pred.numpy(), *gt.shape[-2:])
    want2, n_want2 = mo.batched(gt.numpy(), up, mask.cpu().numpy())
    np.testing.assert_array_equal(n2.cpu().numpy(), n_want2)
    _close(_host(m2), want2)
    up_d = F.interpolate(pred.to(DEV).unsqueeze(1), size=gt.shape[-2:], mode="nearest").squeeze(1)
    _close(_host(metrics.masked_depth_metrics(gt.to(DEV), up_d, mask)), mo.pooled(gt.numpy(), up, mask.cpu().numpy()))


@pytest.mark.gpu
def test_nearest_index_map_equals_aten():
    g = torch.Generator().manual_seed(0)
    for (h, w), (H, W) in [((192, 256), (480, 640)), ((24, 32), (48, 64)), ((16, 20), (40, 50)), ((37, 53), (101, 149)),
                           ((60, 80), (45, 70)), ((7, 9), (7, 9)), ((5, 3), (17, 11)), ((96, 128), (480, 640))]:
        pred = torch.rand((2, 1, h, w), generator=g).to(DEV)
        want = F.interpolate(pred, size=(H, W), mode="nearest").squeeze(1)
        assert torch.equal(metrics._gather(pred, H, W), want), ((h, w), (H, W))


@pytest.mark.gpu
def test_bits_do_not_depend_on_run_batch_or_alignment():
    gt, pred = _scan_maps()
    gt, pred = gt.to(DEV), pred.to(DEV)
    a = metrics.score_block(gt, pred)
    b = metrics.score_block(gt, pred)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    block, counts = metrics.split_block(a, 8)
    H, W = gt.shape[-2:]
    for i in range(8):
        one, c1 = metrics.split_block(metrics.score_block(gt[i:i + 1], pred[i:i + 1]), 1)
        assert torch.equal(one.view(torch.int32), block[i:i + 1].view(torch.int32)) and c1.item() == counts[i].item()
    # a ground truth that is not 16-byte aligned takes the scalar loads: same bits
    store = torch.empty(H * W + 1, device=DEV)
    store[1:] = gt[3].flatten()
    one, _ = metrics.split_block(metrics.score_block(store[1:].view(1, H, W), pred[3:4]), 1)
    assert torch.equal(one.view(torch.int32), block[3:4].view(torch.int32))


@pytest.mark.gpu
def test_scoring_does_not_synchronise():
    gt, pred = _scan_maps(B=2)
    gt, pred = gt.to(DEV).unsqueeze(1), pred.to(DEV).unsqueeze(1)
    metrics.score_frames(gt, pred)   # warm: library load
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        metrics.score_frames(gt, pred)
        metrics.compute_depth_metrics(gt.flatten(), gt.flatten())
        metrics.masked_depth_metrics(gt, gt, gt > 1.0)
    finally:
        torch.cuda.set_sync_debug_mode(0)


@pytest.mark.gpu
def test_depth_model_compute_metrics_both_branches():
    B, h, w = 2, 48, 64
    sc = synthetic.raycast_scene(B, h, w, seed=5, holes=0.02)
    full = synthetic.raycast_scene(B, 2 * h, 2 * w, seed=5, holes=0.02)["depths"]
    pred = synthetic.raycast_scene(B, h, w, seed=5, noise=0.03)["depths"].float().unsqueeze(1).to(DEV)
    depth = sc["depths"].float().unsqueeze(1).to(DEV)
    full = full.float().unsqueeze(1).to(DEV)
    cur = {"depth_b1hw": depth, "mask_b_b1hw": depth > 0.5, "full_res_depth_b1hw": full,
           "full_res_mask_b_b1hw": full > 0.7}
    outputs = {"depth_pred_s0_b1hw": pred}
    holder = types.SimpleNamespace()
    lo = dm.DepthModel.compute_metrics(holder, cur, outputs, "val")
    assert list(lo) == list(mo.KEYS) and all(v.dim() == 0 for v in lo.values())
    _close(_host(lo), mo.pooled(depth.cpu().numpy(), pred.cpu().numpy(), cur["mask_b_b1hw"].cpu().numpy()))
    for phase in ("train", "val"):
        got = dm.DepthModel.compute_metrics(holder, cur, outputs, phase, high_res_validation=True)
        if phase == "train":
            _close(_host(got), _host(lo), rtol=0, rtol_log=0)
            continue
        up = F.interpolate(pred, full.shape[-2:], mode="bilinear", align_corners=False)
        _close(_host(got), mo.pooled(full.cpu().numpy(), up.cpu().numpy(), cur["full_res_mask_b_b1hw"].cpu().numpy()))


class _Recorder:
    """The model as evaluate() sees it, keeping every prediction it returns."""

    def __init__(self, model):
        self.model, self.preds = model, []

    def parameters(self):
        return self.model.parameters()

    def __call__(self, *args, **kwargs):
        out = self.model(*args, **kwargs)
        self.preds.append(out["depth_pred_s0_b1hw"].squeeze(1).cpu())
        return out


def _frames(n, K, h, w, seed):
    """n frames (one (cur, src) each, no batch dimension) of a synthetic scan with full-resolution gt at 4h x 4w."""
    cur, src = synthetic.training_batch(n, K, h, w, seed=seed)
    hi = synthetic.raycast_scene(n * (K + 1), 4 * h, 4 * w, seed=seed)
    Kf = torch.eye(4).repeat(n * (K + 1), 1, 1)
    Kf[:, :3, :3] = hi["K"]
    idx = torch.arange(n) * (K + 1)
    cur["full_res_depth_b1hw"] = hi["depths"][idx].float().unsqueeze(1)
    cur["K_full_depth_b44"] = Kf[idx]
    return [({k: v[i] for k, v in cur.items()}, {k: v[i] for k, v in src.items()}) for i in range(n)]


@pytest.mark.gpu
def test_evaluate_end_to_end(tmp_path):
    from simplerecon_amd.tsdf import OurFuser
    K, h, w = 3, 32, 48
    opts = dm.default_options(image_width=2 * w, image_height=2 * h, model_num_views=K + 1, matching_num_depth_bins=8)
    model = dm.DepthModel(opts)
    for i, m in enumerate((model.encoder, model.matching_model, model.cost_volume_net, model.depth_decoder,
                           model.cost_volume.mlp)):
        synthetic.seeded_fill_(m, seed=21 + i)
    model = model.to(DEV).eval()
    rec = _Recorder(model)
    scans = [("scene_a", _frames(5, K, h, w, seed=1)), ("scan/b", _frames(3, K, h, w, seed=2))]
    bounds = dict(xmin=-3.0, xmax=3.0, ymin=-2.0, ymax=2.0, zmin=-3.0, zmax=3.0)
    frame_avg, scene_avg = evaluate(rec, scans, str(tmp_path), "synthetic", batch_size=2, run_fusion=True,
                                    fuser_factory=lambda scan: OurFuser(bounds=bounds, device=DEV))
    scores = tmp_path / "scores"
    assert sorted(os.listdir(scores)) == ["all_frame_avg_metrics_test.json", "all_scene_avg_metrics_test.json",
                                          "scan_b_metrics.json", "scene_a_metrics.json"]
    meshes = list((tmp_path / "meshes").rglob("*.ply"))
    assert sorted(p.name for p in meshes) == ["scan_b.ply", "scene_a.ply"]
    # the oracle's scoring of the same predictions, batch by batch
    preds = iter(rec.preds)
    all_frames = []
    for scan, frames in scans:
        per_frame = []
        for i in range(0, len(frames), 2):
            gt = torch.stack([c["full_res_depth_b1hw"][0] for c, _ in frames[i:i + 2]]).numpy()
            m, n = mo.score(gt, next(preds).numpy())
            per_frame += [{k: m[k][j] for k in mo.KEYS} for j in range(len(n)) if n[j] > 0]
        data = json.load(open(scores / f"{scan.replace('/', '_')}_metrics.json"))
        assert data["exp_name"] == "synthetic" and data["metrics_type"] == f"scene {scan} metrics"
        assert list(data["scores"]) == list(mo.KEYS) + ["model_time"]
        for k in mo.KEYS:
            want = np.array([f[k] for f in per_frame], np.float32).mean()
            np.testing.assert_allclose(data["scores"][k], want, rtol=1e-5 if k == "rmse_log" else 2e-6, err_msg=k)
        all_frames += per_frame
    data = json.load(open(scores / "all_frame_avg_metrics_test.json"))
    assert len(frame_avg.elem_metrics_list) == len(all_frames) and len(scene_avg.elem_metrics_list) == 2
    for k in mo.KEYS:
        want = np.array([f[k] for f in all_frames], np.float32).mean()
        np.testing.assert_allclose(data["scores"][k], want, rtol=1e-5 if k == "rmse_log" else 2e-6, err_msg=k)
