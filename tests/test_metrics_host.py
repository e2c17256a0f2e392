"""Host side of the depth metrics (no GPU): the numpy oracle against the reference's own outputs
(tests/golden/metrics_<case>.npz), ResultsAverager against the reference's printed lines and JSON bytes, the
reference's signatures and key order, the refusal of host tensors and the C ABI's declarations."""
import contextlib
import glob
import inspect
import io
import json
import os
import re

import numpy as np
import pytest
import torch

import metrics_oracle as mo
from simplerecon_amd import metrics
from simplerecon_amd import depth_model as dm
from simplerecon_amd import evaluation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = sorted(os.path.basename(p)[8:-4] for p in glob.glob(os.path.join(GOLDEN, "metrics_*.npz")))


def load(case):
    return dict(np.load(os.path.join(GOLDEN, f"metrics_{case}.npz")))


def oracle_for(g):
    up = mo.upsample_nearest(g["pred"], *g["gt"].shape[-2:])
    if str(g["mode"]) == "batched":
        with np.errstate(invalid="ignore"):
            valid = g["gt"] > np.float32(0.5)
        return mo.batched(g["gt"], up, valid, mult_a=True)
    return mo.pooled(g["gt"], up, g["mask"], mult_a=False), None


def assert_metrics_match(got, g, rtol=1e-5):
    """Counts and NaN / inf positions exactly, values to rtol."""
    n = g.get("n_valid")
    for k in mo.KEYS:
        a, b = np.asarray(got[k], np.float64), np.asarray(g[k], np.float64)
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=k)
        np.testing.assert_array_equal(np.isinf(a), np.isinf(b), err_msg=k)
        np.testing.assert_array_equal(a[np.isinf(a)], b[np.isinf(b)], err_msg=k)
        fin = np.isfinite(b)
        if k[0] == "a" and n is not None:
            # the a-metrics are counts: n * a / 100 is an integer
            np.testing.assert_array_equal(np.round(a[fin] * n[fin] / 100), np.round(b[fin] * n[fin] / 100), err_msg=k)
        np.testing.assert_allclose(a[fin], b[fin], rtol=rtol, atol=0, err_msg=k)


def test_golden_cases_present():
    for c in ("quirk", "quirk_pooled", "thresholds", "min_depth", "nonfinite", "empty_frame", "nn_1x", "nn_2x",
              "nn_2p5x", "nn_odd", "nn_down", "pooled_mask", "pooled_nan", "pooled_empty", "pooled_nn"):
        assert c in CASES
    for p in glob.glob(os.path.join(GOLDEN, "metrics_*")):
        assert os.path.getsize(p) < 1 << 20


@pytest.mark.parametrize("case", CASES)
def test_oracle_matches_reference(case):
    g = load(case)
    got, n = oracle_for(g)
    if n is not None:
        np.testing.assert_array_equal(n, g["n_valid"])
    assert_metrics_match(got, g)


def test_quirk_frame_values():
    g = load("quirk")
    assert np.isclose(g["a5"][0], 100 / 3, rtol=1e-6)
    for k in ("a10", "a25", "a0", "a1", "a2", "a3"):
        assert g[k][0] == 50.0
    for k in ("abs_diff", "abs_rel", "sq_rel", "rmse", "rmse_log"):
        assert np.isposinf(g[k][0])


def test_nearest_index_matches_aten():
    for n_in, n_out in [(24, 48), (16, 40), (37, 101), (53, 149), (60, 45), (80, 70), (192, 480), (256, 640), (7, 7),
                        (5, 3), (3, 17)]:
        x = torch.arange(n_in, dtype=torch.float32).view(1, 1, 1, n_in)
        want = torch.nn.functional.interpolate(x, size=(1, n_out), mode="nearest").view(-1).long().numpy()
        np.testing.assert_array_equal(mo.nearest_index(n_in, n_out), want)


# ---------------------------------------------------------------------------------------------- averager ----------
def _replay(golden, as_tensor, directory):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        all_frame = metrics.ResultsAverager("exp", "frame metrics")
        all_scene = metrics.ResultsAverager("exp", "scene metrics")
        for scan, frames in golden["scenes"]:
            scene = metrics.ResultsAverager("exp", f"scene {scan} metrics")
            for v in frames:
                e = {k: (as_tensor(x) if k != "model_time" else x) for k, x in v.items()}
                scene.update_results(e)
                all_frame.update_results(e)
            scene.compute_final_average()
            all_scene.update_results(scene.final_metrics)
            print("\nScene metrics:")
            scene.print_sheets_friendly(include_metrics_names=True)
            scene.output_json(os.path.join(directory, f"{scan.replace('/', '_')}_metrics.json"))
            print("\nRunning frame metrics:")
            all_frame.print_sheets_friendly(include_metrics_names=False, print_running_metrics=True)
        print("\nFinal metrics:")
        all_scene.compute_final_average()
        all_scene.pretty_print_results(print_running_metrics=False)
        all_scene.print_sheets_friendly(include_metrics_names=True, print_running_metrics=False)
        all_scene.output_json(os.path.join(directory, "all_scene_avg_metrics_test.json"))
        print("")
        all_frame.compute_final_average()
        all_frame.pretty_print_results(print_running_metrics=False)
        all_frame.print_sheets_friendly(include_metrics_names=True, print_running_metrics=False)
        all_frame.output_json(os.path.join(directory, "all_frame_avg_metrics_test.json"))
        all_frame.compute_final_average(ignore_nans=True)
        all_frame.pretty_print_results(print_exp_name=False, print_running_metrics=True)
        empty = metrics.ResultsAverager("exp", "empty")
        empty.compute_final_average()
        empty.print_sheets_friendly()
        empty.pretty_print_results()
        empty.output_json(os.path.join(directory, "empty.json"))
    files = {f: open(os.path.join(directory, f)).read() for f in sorted(os.listdir(directory))}
    return buf.getvalue(), files


@pytest.mark.parametrize("kind", ["torch", "numpy"])
def test_results_averager_reproduces_reference_output(tmp_path, kind):
    golden = json.load(open(os.path.join(GOLDEN, "metrics_averager.json")))
    conv = (lambda x: torch.tensor(x, dtype=torch.float32)) if kind == "torch" else np.float32
    out, files = _replay(golden, conv, str(tmp_path))
    assert out == golden["stdout"]
    assert files == golden["files"]


def test_results_averager_methods():
    names = ["update_results", "compute_final_average", "print_sheets_friendly", "pretty_print_results", "output_json"]
    for n in names:
        assert callable(getattr(metrics.ResultsAverager, n))
    p = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert p(metrics.ResultsAverager.__init__) == ["self", "exp_name", "metrics_name"]
    assert p(metrics.ResultsAverager.compute_final_average) == ["self", "ignore_nans"]
    assert p(metrics.ResultsAverager.print_sheets_friendly) == ["self", "print_exp_name", "include_metrics_names",
                                                                "print_running_metrics"]
    assert p(metrics.ResultsAverager.pretty_print_results) == ["self", "print_exp_name", "print_running_metrics"]
    assert p(metrics.ResultsAverager.output_json) == ["self", "filepath", "print_running_metrics"]


# ----------------------------------------------------------------------------------------- API surface ------------
def test_reference_signatures_and_keys():
    p = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert p(metrics.compute_depth_metrics) == ["gt", "pred", "mult_a"]
    assert p(metrics.compute_depth_metrics_batched) == ["gt_bN", "pred_bN", "valid_masks_bN", "mult_a"]
    assert inspect.signature(metrics.compute_depth_metrics).parameters["mult_a"].default is False
    sig = inspect.signature(metrics.score_frames).parameters
    assert list(sig) == ["depth_gt_b1HW", "depth_pred_b1hw", "min_depth", "mask_b1HW", "mult_a"]
    assert sig["min_depth"].default == 0.5 and sig["mult_a"].default is True
    assert metrics.METRIC_KEYS == mo.KEYS
    assert p(dm.DepthModel.compute_metrics) == ["self", "cur_data", "outputs", "phase", "high_res_validation"]
    assert p(evaluation.evaluate)[:4] == ["model", "scans", "output_dir", "name"]


def test_host_tensors_and_non_fp32_are_refused():
    from simplerecon_amd._lib import HipLibraryError
    gt, pred = torch.ones(2, 1, 4, 4), torch.ones(2, 1, 4, 4)
    with pytest.raises(HipLibraryError):
        metrics.score_frames(gt, pred)
    with pytest.raises(HipLibraryError):
        metrics.compute_depth_metrics(gt.flatten(), pred.flatten())
    with pytest.raises(HipLibraryError):
        metrics.compute_depth_metrics_batched(gt.view(2, -1), pred.view(2, -1), torch.ones(2, 16, dtype=torch.bool))
    with pytest.raises(TypeError):
        metrics.score_frames(gt.double(), pred)
    with pytest.raises(TypeError):
        metrics.compute_depth_metrics(gt.half(), pred.half())


def test_header_declares_depth_metrics():
    src = open(os.path.join(ROOT, "include", "simplerecon_hip.h")).read()
    assert "depth metrics" in src
    for sym in ("sr_depth_metrics_workspace_bytes", "sr_depth_metrics", "sr_depth_metrics_gather"):
        assert re.search(rf"\b{sym}\s*\(", src)
    for rule in ("nanmean", "1.05f", "1.953125f", "mult_a", "SR_METRICS_MAX_PIXELS", "SR_ERR_WORKSPACE_TOO_SMALL"):
        assert rule in src
