"""Host-side checks of tests/bwd_cases.py (no GPU): the case tables of tests/test_gpu_bwd_shapes.py reach the code paths
they are listed for, and the kink mask zeroes only a sliver of every cotangent."""
import pytest
import torch

import bwd_cases as bc
from simplerecon_amd import _lib

CONV_CPU_FLOPS = 5e9     # float64 forward on the CPU in a few seconds
NORM_CPU_ELEMS = 4e6


@pytest.mark.parametrize("case", bc.CONV_CASES, ids=[c["name"] for c in bc.CONV_CASES])
def test_conv_case_reaches_its_plan(case):
    """The restated plan equals the library's (workspace = blocks * per * k^2 * 64 * 64 * 4 bytes, a host-only query) and the
    row has the property it is in the table for."""
    lib = _lib.lib()
    geo = bc.conv_geometry(case)
    if geo["pads"] is None:
        nws = lib.sr_conv_wgrad_workspace_bytes(case["B"], case["H"], case["W"], case["ci"], case["co"], case["k"], case["s"])
    else:
        nws = lib.sr_conv_wgrad_padded_workspace_bytes(case["B"], geo["Ho"], geo["Wo"], case["ci"], case["co"], case["k"])
    assert nws == bc.wgrad_workspace_bytes(geo, case["k"]), geo
    assert case["prop"](geo), geo
    if case["co"] % 4 != 0:
        assert bc.bias_grad_chunks(geo["pixels"]) == 512


def test_every_gradient_appears_at_a_multi_item_size():
    multi = [c for c in bc.CONV_CASES if (lambda g: g["items"] > g["per"])(bc.conv_geometry(c))]
    assert any(c["bias"] for c in multi) and any(c["res"] for c in multi) and any(c["slope"] is not None for c in multi)
    assert any(c["s"] == 2 for c in multi) and any(c["k"] == 1 for c in multi)
    # the reduce kernel: tail only (per <= 3), 4-way loop with a tail (per > 4, per % 4 != 0), 4-way loop alone
    pers = [bc.conv_geometry(c)["per"] for c in bc.CONV_CASES]
    assert any(p <= 3 for p in pers) and any(p > 4 and p % 4 for p in pers) and any(p >= 4 and p % 4 == 0 for p in pers)


@pytest.mark.parametrize("shape", list(bc.NORM_SHAPES))
def test_norm_shape_reaches_its_plan(shape):
    lib = _lib.lib()
    B, C, H, W, _ = bc.NORM_SHAPES[shape]
    for per_image in (0, 1):
        plan = bc.colreduce_plan(H * W if per_image else B * H * W)
        G = B if per_image else 1
        assert lib.sr_norm_workspace_bytes(B, H * W, C, per_image) == (2 * plan["chunks"] * G * C + 2 * G * C) * 4
    plan = bc.colreduce_plan(B * H * W)
    if shape.endswith("_full"):
        assert B * H * W > 262144 and plan["chunk_pix"] > 256 and plan["chunks"] == 1024
    elif shape != "c1536":              # (2 400 pixels: 10 chunks)
        assert plan["chunks"] > 16      # the finishing kernel's 16 chunk lanes take a second trip
    if shape in ("c160", "c1536"):
        assert C > 64


@pytest.mark.parametrize("case", [c for c in bc.CONV_CASES if c["slope"] is not None and bc.conv_flops(c) < CONV_CPU_FLOPS],
                         ids=lambda c: c["name"])
def test_conv_kink_mask_share(case):
    ref = bc.conv_reference(case, bc.conv_inputs(case, "cpu"), backward=False)
    assert 0.0 < ref["share"] <= bc.KINK_SHARE_MAX, ref["share"]


_NORM_SMALL = [c for c in bc.NORM_CASES if c[2] >= 0.0 and
               (lambda s: s[0] * s[1] * s[2] * s[3])(bc.NORM_SHAPES[c[0]]) < NORM_CPU_ELEMS]


@pytest.mark.parametrize("shape,mode,act,dist", _NORM_SMALL, ids=[bc.norm_id(*c) for c in _NORM_SMALL])
def test_norm_kink_mask_share(shape, mode, act, dist):
    ref = bc.norm_reference(mode, act, bc.norm_inputs(shape, dist, "cpu"), backward=False)
    assert ref["share"] <= bc.KINK_SHARE_MAX, ref["share"]


@pytest.mark.parametrize("kind", ["relu_zeros", "plateaus", "quant3"])
def test_tie_inputs_have_tied_windows(kind):
    assert bc.tied_window_share(bc.tie_input(kind, (2, 6, 37, 50), seed=5)) > 0.10


def test_maxblurpool_smallest_maps():
    assert bc.MBP_SMALL == [(h, w) for h in (4, 5, 6) for w in (4, 5, 6)]
    for h, w in bc.MBP_SMALL:
        assert bc.maxblurpool_reference(torch.zeros((1, 2, h, w), dtype=torch.float64)).shape[2:] == ((h - 2) // 2 + 1, (w - 2) // 2 + 1)
