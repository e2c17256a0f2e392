"""The split-precision format as a value.  The Winograd F(2x2) pack and launch take it as an argument (`split_format`: 0 fp32,
1 bf16 pieces, 2 f16 pieces) and do not look at the option SR_WINO_SPLIT, which is only where a host keeps its choice; the
metadata-MLP entry points read SR_MLP_SPLIT once per call, and the manager falls back from the in-place entry point when that
one reading says split.  Raw C ABI at the smallest shapes at which the split kernel can still go wrong."""
import ctypes as C

import pytest
import torch

import volume_cases as vc
from simplerecon_amd import _lib, ops
from simplerecon_amd import cost_volume as cv

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INVALID = 1
# (B, Cin, H, W, Cout, residual and bias): one 8x16 region and one 16-channel slab; partial regions (12x20 = 2 x 2 regions of
# 8x16), two slabs, two images, the whole epilogue
SHAPES = [(1, 16, 8, 16, 32, False), (2, 32, 12, 20, 64, True)]
FORMATS = {"": 0, "bf16": 1, "f16": 2}


def _layer(shape):
    b, ci, h, w, co, extras = shape
    g = torch.Generator().manual_seed(ci + co + h)
    conv = torch.nn.Conv2d(ci, co, 3, padding=1, bias=extras)
    with torch.no_grad():
        for p in conv.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.1)
    nhwc = lambda c: torch.randn((b, c, h, w), generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    return conv.to(DEV), nhwc(ci), nhwc(co) if extras else None


def _pack(conv, fmt, wp=None):
    lib = _lib.lib()
    co, ci = conv.out_channels, conv.in_channels
    if wp is None:
        wp = torch.empty(lib.sr_wino_packed_weight_floats(co, ci), dtype=torch.float32, device=DEV)
    rc = lib.sr_wino_pack_weights(_lib.ptr(conv.weight.detach().contiguous()), co, ci, fmt, _lib.ptr(wp), _lib.stream_ptr())
    return rc, wp


def _launch(conv, x, res, wp, fmt, out):
    b, ci, h, w = x.shape
    rsb, rsp = ops._strides(res) if res is not None else (0, 0)
    bias = conv.bias.detach() if conv.bias is not None else None
    return _lib.lib().sr_conv3x3_wino_splitk_nhwc_fwd(
        _lib.ptr(x), *ops._strides(x), _lib.ptr(wp), _lib.ptr(bias), _lib.ptr(res), rsb, rsp, _lib.ptr(out), *ops._strides(out),
        b, h, w, ci, conv.out_channels, C.c_float(0.2), fmt, None, 0, _lib.stream_ptr())


def _raw(conv, x, res, fmt):
    rc, wp = _pack(conv, fmt)
    assert rc == 0
    out = ops.empty_nhwc(x.shape[0], conv.out_channels, x.shape[2], x.shape[3], DEV)
    assert _launch(conv, x, res, wp, fmt, out) == 0
    torch.cuda.synchronize()
    return out


@pytest.fixture
def by_option(monkeypatch, sr_option):
    """mode -> ops.conv2d of the layer under SR_WINO_SPLIT = mode, on F(2x2) (the form the split kernels restate)."""
    monkeypatch.setattr(ops, "WINO4_MODE", 0)

    def run(mode, conv, x, res):
        sr_option("SR_WINO_SPLIT", mode)
        with torch.inference_mode():
            y = ops.conv2d(x, conv, residual=res, leaky=0.2)
        torch.cuda.synchronize()
        return y
    return run


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_the_argument_selects_the_format_and_the_option_does_not(shape, by_option, sr_option):
    conv, x, res = _layer(shape)
    want = {mode: by_option(mode, conv, x, res) for mode in FORMATS}
    assert not torch.equal(want["f16"], want[""]) and not torch.equal(want["bf16"], want["f16"])
    sr_option("SR_WINO_SPLIT", 0)
    for mode in ("f16", "bf16"):   # (a) split formats by argument while the option is off
        assert torch.equal(_raw(conv, x, res, FORMATS[mode]), want[mode]), mode
    sr_option("SR_WINO_SPLIT", "f16")   # (b) the fp32 format by argument while the option says f16
    assert torch.equal(_raw(conv, x, res, 0), want[""])


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_an_unknown_format_is_refused_and_nothing_is_written(shape):
    conv, x, res = _layer(shape)   # (c)
    rc, wp = _pack(conv, 0)
    assert rc == 0
    filled = torch.full_like(wp, 7.0)
    assert _pack(conv, 3, filled)[0] == INVALID
    out = torch.full((x.shape[0], conv.out_channels, x.shape[2], x.shape[3]), 7.0, device=DEV).contiguous(
        memory_format=torch.channels_last)
    assert _launch(conv, x, res, wp, 3, out) == INVALID
    torch.cuda.synchronize()
    assert bool((filled == 7.0).all()) and bool((out == 7.0).all())


def test_the_sweep_falls_back_from_the_in_place_entry_point_under_split(monkeypatch, sr_option):
    """(d) channels-last features under SR_MLP_SPLIT: the split kernel reads cur planar, so the manager hands sr_mlp_volume_fwd
    contiguous copies -- by its look at the mirror, and, when the library was set behind the mirror's back, by the in-place
    entry point's SR_ERR_UNSUPPORTED.  Bit-equal to the same call on contiguous inputs either way."""
    case = min(vc.MLP_CASES, key=lambda c: c["B"] * c["D"] * c["h"] * c["w"])   # fewest (pixel, plane) evaluations
    B, K = case["B"], case["K"]
    inp = vc.to_device(vc.inputs(case), DEV)
    mgr = vc.manager(case).to(DEV)
    both = torch.cat([inp["cur_feats"], inp["src_feats"].flatten(0, 1)]).contiguous(memory_format=torch.channels_last)
    cur, src = both[:B], both[B:].unflatten(0, (B, K))
    assert cv.dense_channels_last_pair(cur, src) and inp["cur_feats"].is_contiguous() and inp["src_feats"].is_contiguous()
    real, calls = _lib.lib(), []

    class Counting:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith("sr_mlp_volume_fwd"):
                return fn

            def counted(*args):
                rc = fn(*args)
                calls.append((name, rc))
                return rc
            return counted
    monkeypatch.setattr(_lib, "lib", lambda: Counting())

    def run(cur_feats, src_feats):
        del calls[:]
        with torch.inference_mode():
            vol, lowest, _, mask = mgr(return_mask=True, **dict(inp, cur_feats=cur_feats, src_feats=src_feats))
        torch.cuda.synchronize()
        return vol, lowest, mask, list(calls)
    fp32 = run(cur, src)
    assert fp32[3] == [("sr_mlp_volume_fwd_nhwc", 0)]
    sr_option("SR_MLP_SPLIT", "f16")
    want = run(inp["cur_feats"], inp["src_feats"])
    assert want[3] == [("sr_mlp_volume_fwd", 0)] and not torch.equal(want[0], fp32[0])
    got = run(cur, src)
    assert got[3] == [("sr_mlp_volume_fwd", 0)]
    assert all(torch.equal(g, t) for g, t in zip(got[:3], want[:3]))
    # the library in f16 mode, the mirror still at 0 (a host that drives sr_option_set by other means)
    sr_option("SR_MLP_SPLIT", 0)
    oid = real.sr_option_id(b"SR_MLP_SPLIT")
    try:
        assert real.sr_option_set(oid, 2, None) == 0 and _lib.get_option("SR_MLP_SPLIT") == 0
        got = run(cur, src)
    finally:
        real.sr_option_set(oid, 0, None)
    assert got[3] == [("sr_mlp_volume_fwd_nhwc", _lib.ERR_UNSUPPORTED), ("sr_mlp_volume_fwd", 0)]
    assert all(torch.equal(g, t) for g, t in zip(got[:3], want[:3]))
