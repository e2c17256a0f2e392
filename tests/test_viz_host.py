"""Host side of simplerecon_amd.visualization (no GPU): the shipped turbo table against matplotlib, and the argument
checks -- host tensors are refused (no CPU path), wrong shapes and dtypes raise naming the argument."""
import glob
import os

import numpy as np
import pytest
import torch

from simplerecon_amd import visualization as viz
from simplerecon_amd._lib import HipLibraryError

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_turbo_table_equals_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    want = torch.Tensor(matplotlib.colormaps["turbo"](np.linspace(0, 1, 256))[:, :3])
    got = viz.colormap_table("turbo")
    assert got.dtype == torch.float32 and tuple(got.shape) == (256, 3)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_other_tables_come_from_matplotlib():
    matplotlib = pytest.importorskip("matplotlib")
    want = torch.Tensor(matplotlib.colormaps["viridis"](np.linspace(0, 1, 256))[:, :3])
    assert torch.equal(viz.colormap_table("viridis"), want)


def test_unknown_colormap_raises():
    pytest.importorskip("matplotlib")
    with pytest.raises(ValueError, match="no_such_map"):
        viz.colormap_table("no_such_map")
    with pytest.raises(ValueError, match="colormap"):
        viz._table(torch.zeros(255, 3), True, torch.device("cpu"))
    with pytest.raises(TypeError, match="colormap"):
        viz._table(torch.zeros(256, 3, dtype=torch.float64), True, torch.device("cpu"))


def test_host_tensors_are_refused():
    img = torch.rand(1, 6, 8)
    for call in (lambda: viz.colormap_image(img), lambda: viz.colormap_u8(img), lambda: viz.colormap_image(img[None]),
                 lambda: viz.value_range(img), lambda: viz.normals_u8(torch.rand(2, 3, 6, 8)),
                 lambda: viz.normals_image(torch.rand(2, 3, 6, 8)), lambda: viz.color_u8(torch.rand(2, 3, 6, 8)),
                 lambda: viz.color_image(torch.rand(3, 6, 8))):
        with pytest.raises(HipLibraryError):
            call()
    cur = {"full_res_depth_b1hw": torch.rand(2, 1, 6, 8), "image_b3hw": torch.rand(2, 3, 6, 8)}
    out = {"depth_pred_s0_b1hw": torch.rand(2, 1, 3, 4), "lowest_cost_bhw": torch.rand(2, 3, 4)}
    with pytest.raises(HipLibraryError):
        viz.quick_viz_export("unused", out, cur, 0, cur["full_res_depth_b1hw"] > 0.5, 2)


def test_wrong_shapes_and_dtypes_name_the_argument():
    with pytest.raises(ValueError, match="image_1hw"):
        viz.colormap_image(torch.rand(2, 6, 8))
    with pytest.raises(ValueError, match="image_1hw"):
        viz.colormap_image(torch.rand(2, 3, 6, 8))
    with pytest.raises(ValueError, match="image_1hw"):
        viz.colormap_u8(torch.rand(6, 8))
    with pytest.raises(TypeError, match="image_1hw"):
        viz.colormap_image(torch.rand(1, 6, 8).double())
    with pytest.raises(TypeError, match="image_1hw"):
        viz.colormap_image(np.zeros((1, 6, 8), np.float32))
    with pytest.raises(ValueError, match="normals_b3hw"):
        viz.normals_u8(torch.rand(2, 1, 6, 8))
    with pytest.raises(TypeError, match="normals_b3hw"):
        viz.normals_image(torch.rand(2, 3, 6, 8).half())
    with pytest.raises(ValueError, match="image_b3hw"):
        viz.color_u8(torch.rand(2, 4, 6, 8))
    with pytest.raises(TypeError, match="image_b3hw"):
        viz.color_u8(torch.zeros(2, 3, 6, 8, dtype=torch.uint8))
    # masks and ranges are looked at before anything is launched
    like = torch.rand(1, 6, 8)
    with pytest.raises(TypeError, match="mask_1hw"):
        viz._mask("mask_1hw", torch.zeros(1, 6, 8, dtype=torch.int64), like)
    with pytest.raises(ValueError, match="mask_1hw"):
        viz._mask("mask_1hw", torch.zeros(1, 6, 7), like)
    with pytest.raises(TypeError, match="vmin"):
        viz._bound("vmin", torch.zeros(1, dtype=torch.float64), 1, like.device)
    with pytest.raises(ValueError, match="vmax"):
        viz._bound("vmax", torch.zeros(3), 2, like.device)
    with pytest.raises(TypeError, match="vmax"):
        viz._bound("vmax", "5", 2, like.device)
    with pytest.raises(HipLibraryError, match="vmin"):
        viz._bound("vmin", torch.zeros(1), 1, like.device)


def test_fixtures_hold_every_case_of_the_issue():
    cm = sorted(os.path.basename(p)[len("viz_cm_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "viz_cm_*.npz")))
    assert cm == sorted(["plain", "mask01", "mask_fraction", "noflip", "viridis", "given_range", "bin_edges",
                         "bin_edges_255", "nonfinite", "equal_range", "nan_valid", "multi_block", "denormal"])
    quick = sorted(os.path.basename(p)[len("viz_quick_"):-len(".npz")]
                   for p in glob.glob(os.path.join(GOLDEN, "viz_quick_*.npz")))
    assert quick == sorted(["ordinary", "sample_invalid", "sample_constant", "nothing_valid"])
    counts = {n: len(np.load(os.path.join(GOLDEN, f"viz_quick_{n}.npz"))["names"]) for n in quick}
    assert counts == {"ordinary": 12, "sample_invalid": 11, "sample_constant": 11, "nothing_valid": 9}
    g = np.load(os.path.join(GOLDEN, "viz_cm_equal_range.npz"))
    assert len(np.unique(g["out"].reshape(3, -1).T, axis=0)) == 2          # a division by zero: two colours
    g = np.load(os.path.join(GOLDEN, "viz_cm_nan_valid.npz"))
    assert np.isnan(g["vmin_out"]) and np.isnan(g["vmax_out"])
