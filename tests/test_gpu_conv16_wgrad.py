"""The 16-bit-operand weight gradient of the autocast training path (csrc/sr_conv16_wgrad.hip): sr_conv16_wgrad_nhwc on
v_mfma_f32_32x32x16_* with transposed LDS reads, fp32 accumulation and an ordered slab reduction, and sr_act_bwd_bias16_nhwc,
the elementwise backward pass on 16-bit tensors.

(a) exact small integers, bit for bit against the fp64 weight gradient -- the fragment-layout test (patterns asymmetric in every
    index), with NaN in every byte around the operands, in the output and in the workspace;
(b) the (2,64,33,64,160) case really reduces several partial slabs per block;
(c) random operands against fp64 with a DERIVED elementwise bound (fp32 accumulation of N exact products in any order);
(d) two launches give the same bits;
(e) refusals launch nothing;
(f) sr_act_bwd_bias16_nhwc: grad_pre bit for bit, d_bias inside its bound and deterministic;
(g) the conv stack trains under experimental.autocast_mfma16(mode=2, wgrad=2) on the new kernels and agrees with the fp32 run."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from parity import rel_err
from simplerecon_amd import _lib, autograd_ops, experimental, ops, synthetic
from simplerecon_amd.networks import CVEncoder, DepthDecoderPP

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.float16, torch.bfloat16]
IO = {torch.float16: 1, torch.bfloat16: 2}
SHAPES = [(1, 8, 5, 7, 8), (3, 24, 17, 23, 40), (2, 64, 33, 64, 160), (1, 40, 6, 9, 64), (1, 16, 4, 45, 16)]   # (B, Ci, H, W, Co)
FORMS = [(1, 1), (3, 1), (3, 2)]                                                                               # (k, stride)
SR_ERR_INVALID_ARGUMENT, SR_ERR_UNSUPPORTED = 1, 2
NAN = float("nan")


def _out_hw(h, w, k, stride):
    return (h + 2 * (k // 2) - k) // stride + 1, (w + 2 * (k // 2) - k) // stride + 1


def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def _sliced(t, dt):
    """`t` ([B,C,H,W], CPU) as the channel slice [8, 8 + C) of a channels-last device tensor 16 channels wider whose other
    channels hold NaN."""
    b, c, h, w = t.shape
    wide = _nhwc(torch.full((b, c + 16, h, w), NAN, dtype=dt, device=DEV))
    view = wide[:, 8:8 + c]
    view.copy_(t.to(DEV).to(dt))
    return view


def _workspace(shape, k, stride, fill=NAN):
    B, ci, H, W, co = shape
    n = _lib.lib().sr_conv16_wgrad_workspace_bytes(B, H, W, ci, co, k, stride)
    assert n > 0 and n % 16 == 0
    return torch.full((n // 4,), fill, dtype=torch.float32, device=DEV), n


def _wgrad_rc(x, g, dw, k, stride, ws, nws, io=None, x_ptr=True, g_ptr=True, dw_ptr=True, ws_ptr=True):
    """The raw return code of sr_conv16_wgrad_nhwc on channels-last views."""
    b, ci, h, w = x.shape
    co = g.shape[1]
    io = IO[x.dtype] if io is None else io
    return _lib.lib().sr_conv16_wgrad_nhwc(_lib.ptr(x) if x_ptr else None, *ops._strides(x), _lib.ptr(g) if g_ptr else None,
                                           *ops._strides(g), _lib.ptr(dw) if dw_ptr else None, b, h, w, ci, co, k, stride, io,
                                           _lib.ptr(ws) if ws_ptr else None, nws, _lib.stream_ptr(x.device))


def _idx(*shape):
    return torch.meshgrid(*[torch.arange(n, dtype=torch.int64) for n in shape], indexing="ij")


def _wgrad64(x, g, k, stride):
    """The fp64 weight gradient, by autograd through F.conv2d on the CPU."""
    co, ci = g.shape[1], x.shape[1]
    w = torch.zeros((co, ci, k, k), dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, None, stride=stride, padding=k // 2).backward(g.double())
    return w.grad.detach()


@functools.lru_cache(maxsize=None)
def _integer_case(shape, k, stride):
    """Integer operands (fp64, CPU): x in [-3, 3], g in [-2, 2], asymmetric in every index, and their exact weight gradient."""
    B, ci, H, W, co = shape
    ho, wo = _out_hw(H, W, k, stride)
    b, c, y, x = _idx(B, ci, H, W)
    xs = ((7 * b + 3 * y + 5 * x + c) % 7 - 3).double()
    gb, gc, gy, gx = _idx(B, co, ho, wo)
    gs = ((3 * gb + 4 * gc + 2 * gy + gx) % 5 - 2).double()
    return xs, gs, _wgrad64(xs, gs, k, stride)


@pytest.mark.parametrize("k,stride", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dt", DTYPES)
def test_exact_integers_bit_for_bit(dt, shape, k, stride):
    """|sum| <= 6 B Ho Wo < 2^24: every product and partial sum is exact whatever the order, so d_weight must EQUAL the fp64
    weight gradient.  Both operands are channel slices of wider tensors whose other channels hold NaN; d_weight and the
    workspace start as NaN: a result that touched any of it is not finite."""
    xs, gs, want = _integer_case(shape, k, stride)
    assert 6 * gs[:, 0].numel() < 2 ** 24
    x, g = _sliced(xs, dt), _sliced(gs, dt)
    dw = torch.full(want.shape, NAN, dtype=torch.float32, device=DEV)
    ws, nws = _workspace(shape, k, stride)
    _lib.check(_wgrad_rc(x, g, dw, k, stride, ws, nws), "sr_conv16_wgrad_nhwc")
    got = dw.cpu()
    assert bool(torch.isfinite(got).all())
    assert torch.equal(got.double(), want), float((got.double() - want).abs().max())


def test_the_slab_reduction_is_exercised():
    """(2,64,33,64,160) at 3x3 / stride 1: 3 (co, ci) blocks; the documented workspace formula (blocks x slabs x taps x 64 x 64
    x 4 bytes) gives the slabs per block, and there are several -- test (a) on this shape adds them in the second kernel."""
    B, ci, H, W, co = 2, 64, 33, 64, 160
    n = _lib.lib().sr_conv16_wgrad_workspace_bytes(B, H, W, ci, co, 3, 1)
    blocks = -(-co // 64) * -(-ci // 64)
    slabs, rest = divmod(n, blocks * 9 * 64 * 64 * 4)
    assert rest == 0 and slabs >= 2, (n, blocks, slabs)
    assert slabs == min(-(-512 // blocks), B * H * -(-W // 32))


def _random_case(shape, k, stride, dt, seed):
    """x ~ N(0, 1), g ~ N(0, 1 / N) rounded to `dt`: |dW| ~ 1, far from fp16's range (the scaling of test_gpu_conv16's
    _random_case, with the pixel count in the place of the fan-in)."""
    B, ci, H, W, co = shape
    ho, wo = _out_hw(H, W, k, stride)
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((B, ci, H, W), generator=gen).to(dt)
    g = (torch.randn((B, co, ho, wo), generator=gen) * (1.0 / (B * ho * wo) ** 0.5)).to(dt)
    return x, g


@pytest.mark.parametrize("shape,k,stride", [(sh, k, s) for sh in SHAPES for k, s in FORMS] + [((1, 64, 120, 160, 64), 3, 1)])
@pytest.mark.parametrize("dt", DTYPES)
def test_random_data_within_the_derived_bound(dt, shape, k, stride):
    """|dW - R| <= (N + 4) 2^-23 A + 2^-149, elementwise: R the fp64 gradient on the rounded operands, A the fp64 gradient of
    |g| with |x|, N = B Ho Wo -- fp32 accumulation of N exact products in any order; the output is not rounded, so there is
    no u |R| term."""
    x, g = _random_case(shape, k, stride, dt, 11 * shape[1] + shape[4] + k + stride)
    R, A = _wgrad64(x, g, k, stride), _wgrad64(x.abs(), g.abs(), k, stride)
    dw = torch.full(R.shape, NAN, dtype=torch.float32, device=DEV)
    ws, nws = _workspace(shape, k, stride)
    _lib.check(_wgrad_rc(_sliced(x, dt), _sliced(g, dt), dw, k, stride, ws, nws), "sr_conv16_wgrad_nhwc")
    N = g[:, 0].numel()
    bound = (N + 4) * 2.0 ** -23 * A + 2.0 ** -149
    err = (dw.cpu().double() - R).abs()
    worst = float((err / bound).max())
    print(f"conv16 wgrad bound: max err {float(err.max()):.3e}, worst err / bound {worst:.4f}, max |R| {float(R.abs().max()):.2f}")
    assert float(R.abs().max()) < 1000 and worst <= 1.0, worst


@pytest.mark.parametrize("k,stride", FORMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_two_launches_give_the_same_bits(dt, k, stride):
    shape = (2, 64, 33, 64, 160)
    x, g = _random_case(shape, k, stride, dt, 3)
    xd, gd = _nhwc(x.to(DEV)), _nhwc(g.to(DEV))
    outs = []
    for fill in (NAN, 3.0):   # (whatever the workspace and the output held before)
        dw = torch.full((shape[4], shape[1], k, k), fill, dtype=torch.float32, device=DEV)
        ws, nws = _workspace(shape, k, stride, fill)
        _lib.check(_wgrad_rc(xd, gd, dw, k, stride, ws, nws), "sr_conv16_wgrad_nhwc")
        outs.append(dw)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].abs().max()) > 0


def test_refusals_launch_nothing():
    dt = torch.bfloat16
    B, ci, H, W, co = 1, 16, 6, 9, 16
    wide = _nhwc(torch.randn((B, ci + 16, H, W), device=DEV).to(dt))
    x = wide[:, 8:8 + ci]
    gwide = _nhwc(torch.randn((B, co + 16, H, W), device=DEV).to(dt))
    g = gwide[:, 8:8 + co]
    g2 = _nhwc(torch.randn((B, co, 3, 5), device=DEV).to(dt))                      # (stride-2 gradient)
    odd = _nhwc(torch.randn((B, ci + 4, H, W), device=DEV).to(dt))                # pixel stride 20: not a multiple of 8
    dw = torch.full((co, ci, 3, 3), 7.0, dtype=torch.float32, device=DEV)
    dw1 = torch.full((co, ci, 1, 1), 7.0, dtype=torch.float32, device=DEV)
    ws, nws = _workspace((B, ci, H, W, co), 3, 1, fill=7.0)
    U, I = SR_ERR_UNSUPPORTED, SR_ERR_INVALID_ARGUMENT
    cases = [
        (_wgrad_rc(wide[:, 4:4 + ci], g, dw, 3, 1, ws, nws), U),                  # input rows 8 bytes off
        (_wgrad_rc(x, gwide[:, 4:4 + co], dw, 3, 1, ws, nws), U),                 # gradient rows 8 bytes off
        (_wgrad_rc(odd[:, :ci], g, dw, 3, 1, ws, nws), U),                        # a pixel stride of 20
        (_wgrad_rc(x, odd[:, :co], dw, 3, 1, ws, nws), U),
        (_wgrad_rc(wide[:, :12], g, dw, 3, 1, ws, nws), U),                       # Cin = 12
        (_wgrad_rc(x, gwide[:, :12], dw, 3, 1, ws, nws), U),                      # Cout = 12
        (_wgrad_rc(x, g, dw, 3, 1, ws, nws - 1), U),                              # a workspace one byte short
        (_wgrad_rc(x, g, dw, 3, 1, ws.view(torch.uint8)[8:].view(torch.float32), nws), U),   # workspace 8 bytes off
        (_wgrad_rc(x, g, dw, 3, 1, ws, nws, io=0), I),
        (_wgrad_rc(x, g, dw, 3, 1, ws, nws, io=3), I),
        (_wgrad_rc(x, g, dw, 5, 1, ws, nws), I),
        (_wgrad_rc(x, g, dw, 3, 3, ws, nws), I),
        (_wgrad_rc(x, g2, dw1, 1, 2, ws, nws), I),                                # k = 1 at stride 2
        (_wgrad_rc(x, g, dw, 3, 1, ws, nws, x_ptr=False), I),
        (_wgrad_rc(x, g, dw, 3, 1, ws, nws, g_ptr=False), I),
        (_wgrad_rc(x, g, dw, 3, 1, ws, nws, dw_ptr=False), I),
        (_wgrad_rc(x, g, dw, 3, 1, ws, nws, ws_ptr=False), I),
    ]
    torch.cuda.synchronize()
    assert [got for got, _ in cases] == [want for _, want in cases]
    assert bool((dw == 7).all()) and bool((dw1 == 7).all()) and bool((ws == 7).all())
    _lib.check(_wgrad_rc(x, g, dw, 3, 1, ws, nws), "sr_conv16_wgrad_nhwc")          # (the accepted call does write)
    assert not bool((dw == 7).any()) and not bool((ws == 7).all())


def _act_rc(g, out, gp, db, px, c, slope, io, ws, nws):
    return _lib.lib().sr_act_bwd_bias16_nhwc(_lib.ptr(g), 0 if g.dtype == torch.float32 else io, _lib.ptr(out), _lib.ptr(gp),
                                             _lib.ptr(db), px, c, 0.0 if slope is None else slope, io, _lib.ptr(ws), nws,
                                             _lib.stream_ptr(g.device))


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("slope", [None, 0.0, 0.2])
@pytest.mark.parametrize("px,c", [(35, 8), (1000, 8), (35, 40), (1000, 40)])
@pytest.mark.parametrize("g32", [True, False])
@pytest.mark.parametrize("dt", DTYPES)
def test_act_bwd_bias16(dt, g32, px, c, slope, with_bias):
    """grad_pre = (g.float() * where(out > 0, 1, slope)).to(dt) bit for bit (one fp32 multiply, one rounding); d_bias within
    (pixels + 4) 2^-23 sum |term| of the fp64 column sum of the unrounded products (fp32 accumulation in any order), and the same
    bits in two runs."""
    gen = torch.Generator().manual_seed(px + 7 * c + (3 if g32 else 0))
    g = torch.randn((px, c), generator=gen).to(torch.float32 if g32 else dt).to(DEV)
    out = torch.randn((px, c), generator=gen).to(dt).to(DEV)
    out[::3, ::2] = 0.0                                                            # ties: out == 0 takes the slope
    act = slope is not None
    term = g.float() * torch.where(out > 0, 1.0, float(slope)) if act else g.float()
    want = term.to(dt)
    nws = _lib.lib().sr_act_bwd_bias16_workspace_bytes(px, c)
    assert nws > 0 and nws % 16 == 0
    dbs = []
    for fill in (NAN, 3.0):
        gp = torch.full((px, c), NAN, dtype=dt, device=DEV)
        db = torch.full((c,), fill, dtype=torch.float32, device=DEV) if with_bias else None
        ws = torch.full((nws // 4,), fill, dtype=torch.float32, device=DEV) if with_bias else None
        _lib.check(_act_rc(g, out if act else None, gp, db, px, c, slope, IO[dt], ws, nws if with_bias else 0),
                   "sr_act_bwd_bias16_nhwc")
        assert torch.equal(gp.view(torch.int16), want.view(torch.int16))
        dbs.append(db)
    if with_bias:
        t64 = term.double()
        bound = (px + 4) * 2.0 ** -23 * t64.abs().sum(0) + 2.0 ** -149
        err = (dbs[0].double() - t64.sum(0)).abs()
        print(f"act_bwd_bias16: worst err / bound {float((err / bound).max()):.4f}")
        assert bool((err <= bound).all()), float((err / bound).max())
        assert torch.equal(dbs[0].view(torch.int32), dbs[1].view(torch.int32))


def test_act_bwd_bias16_bias_only_leaves_grad_pre_alone():
    """No activation and a NULL grad_pre: only the bias gradient is computed (the 16-bit gradient is its own grad_pre)."""
    dt, px, c = torch.bfloat16, 1000, 40
    g = torch.randn((px, c), generator=torch.Generator().manual_seed(1)).to(dt).to(DEV)
    nws = _lib.lib().sr_act_bwd_bias16_workspace_bytes(px, c)
    ws = torch.full((nws // 4,), NAN, dtype=torch.float32, device=DEV)
    db = torch.full((c,), NAN, dtype=torch.float32, device=DEV)
    _lib.check(_act_rc(g, None, None, db, px, c, None, IO[dt], ws, nws), "sr_act_bwd_bias16_nhwc")
    t64 = g.double()
    assert bool(((db.double() - t64.sum(0)).abs() <= (px + 4) * 2.0 ** -23 * t64.abs().sum(0)).all())


@pytest.mark.parametrize("dt", DTYPES)
def test_conv_stack_trains_on_the_16bit_weight_gradient(dt, monkeypatch):
    """The conv stack of test_conv_stack_trains_on_the_16bit_mfma_kernel (same modules, seeds, sizes, 2^10 loss scale for fp16)
    under experimental.autocast_mfma16(mode=2, wgrad=2): every layer whose forward ran on sr_conv16_nhwc_fwd takes its weight
    gradient on sr_conv16_wgrad_nhwc and its elementwise pass on sr_act_bwd_bias16_nhwc; outputs and parameter gradients agree
    with the fp32 run within that test's tolerances (3e-2 fp16, 2e-1 bf16).  With wgrad=0 no new call appears."""
    before = (autograd_ops.HALF_IO, autograd_ops.MFMA16, autograd_ops.STORE_HALF, autograd_ops.MFMA16_WGRAD)
    torch.manual_seed(0)
    enc = synthetic.seeded_fill_(CVEncoder(16, [8, 12, 16, 24], [16, 24, 32, 48]), seed=1).to(DEV)
    dec = synthetic.seeded_fill_(DepthDecoderPP([6] + enc.num_ch_enc), seed=2).to(DEV)
    gen = torch.Generator().manual_seed(5)
    B, H, W = 2, 32, 48
    vol = torch.randn((B, 16, H, W), generator=gen).to(DEV).requires_grad_(True)
    pyr = [torch.randn((B, c, H >> i, W >> i), generator=gen).to(DEV) for i, c in enumerate([8, 12, 16, 24])]
    f0 = torch.randn((B, 6, 2 * H, 2 * W), generator=gen).to(DEV)
    scale = 2.0 ** 10 if dt == torch.float16 else 1.0

    calls = []
    real_call = _lib.call

    def counting_call(name, device, *args, **kw):
        calls.append((name, args))
        return real_call(name, device, *args, **kw)
    monkeypatch.setattr(_lib, "call", counting_call)

    def step(autocast):
        for m in (enc, dec):
            m.zero_grad(set_to_none=True)
        vol.grad = None
        s = scale if autocast else 1.0
        with torch.autocast("cuda", dtype=dt, enabled=autocast):
            out = dec([f0] + enc(vol, pyr))
            loss = sum(out[f"log_depth_pred_s{i}_b1hw"].float().abs().mean() for i in range(4))
        fwd16 = {tuple(a[11:18]) for name, a in calls if name == "sr_conv16_nhwc_fwd"}   # (B, H, W, Cin, Cout, k, stride)
        (loss * s).backward()
        grads = {n: p.grad / s for m in (enc, dec) for n, p in m.named_parameters() if p.grad is not None}
        return out, grads, vol.grad / s, fwd16

    ref_out, ref_g, ref_dv, _ = step(False)
    assert not any(name.startswith(("sr_conv16", "sr_act_bwd_bias16")) for name, _ in calls)   # fp32: the new code is not reached
    calls.clear()
    with experimental.autocast_mfma16(mode=2):
        step(True)
    names_before = [name for name, _ in calls]
    calls.clear()
    with experimental.autocast_mfma16(mode=2, wgrad=0):
        step(True)
    assert [name for name, _ in calls] == names_before
    assert "sr_conv16_wgrad_nhwc" not in names_before and "sr_act_bwd_bias16_nhwc" not in names_before
    calls.clear()
    with experimental.autocast_mfma16(mode=2, wgrad=2):
        out, gr, dv, fwd16 = step(True)
    assert (autograd_ops.HALF_IO, autograd_ops.MFMA16, autograd_ops.STORE_HALF, autograd_ops.MFMA16_WGRAD) == before
    n_w = sum(name == "sr_conv16_wgrad_nhwc" for name, _ in calls)
    n_a = sum(name == "sr_act_bwd_bias16_nhwc" for name, _ in calls)
    assert n_w > 0 and n_a > 0 and len(fwd16) > 0, (n_w, n_a)
    sup = _lib.lib().sr_conv16_wgrad_supported
    for name, a in calls:
        if name == "sr_conv_wgrad_nhwc":   # (x, strides, g, strides, d_w, B, H, W, Cin, Cout, k, stride, ...)
            assert not (tuple(a[7:14]) in fwd16 and sup(*a[7:14])), a[7:14]
    tol = 3e-2 if dt == torch.float16 else 2e-1
    for i in range(4):
        key = f"log_depth_pred_s{i}_b1hw"
        assert out[key].dtype == dt and torch.isfinite(out[key]).all()
        assert rel_err(out[key].float(), ref_out[key]) < tol, (key, rel_err(out[key].float(), ref_out[key]))
    assert sorted(gr) == sorted(ref_g) and dv.dtype == torch.float32 and torch.isfinite(dv).all()
    assert all(torch.isfinite(v).all() for v in gr.values())

    def l2(a, b):
        return float((a.float() - b).norm() / b.norm().clamp_min(1e-12))
    errs = [l2(gr[n], ref_g[n]) for n in gr]
    print(f"conv16 wgrad stack {dt}: median grad err {np.median(errs):.3e}, max {max(errs):.3e}, wgrad16 launches {n_w}, "
          f"act16 launches {n_a}")
    assert np.median(errs) < tol, (np.median(errs), max(errs))
