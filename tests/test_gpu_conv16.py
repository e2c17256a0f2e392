"""16-bit MFMA convolutions of the autocast training path (csrc/sr_conv16.hip; reference options.py:100-101 `precision: 16`,
train.py:132): out = round_to(out_dtype, act(sum + bias + residual)) with fp16 / bf16 operands on v_mfma_f32_32x32x16_*,
fp32 accumulation, one rounding on the way out.

(a) exact small integers, bit for bit against an fp64 convolution -- the fragment-layout test (patterns asymmetric in every
    index: a row <-> column or tap swap cannot pass);
(b) random operands against fp64 with a DERIVED elementwise bound (one output rounding + fp32 accumulation in any order);
(c) two launches give the same bits;
(d) refusals launch nothing;
(e) the conv stack trains under torch.autocast + experimental.autocast_mfma16(mode=2): forward and data gradient run on the
    new kernel and agree with the fp32 run to the 16-bit-activation tolerances of test_gpu_half_io.py."""
import ctypes as C
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
SHAPES = [(1, 8, 5, 7, 8), (3, 24, 17, 23, 40), (2, 64, 33, 64, 160), (1, 40, 6, 9, 64)]     # (B, Ci, H, W, Co)
FORMS = [(1, 1), (3, 1), (3, 2)]                                                              # (k, stride)
SR_ERR_INVALID_ARGUMENT, SR_ERR_UNSUPPORTED = 1, 2


def _pack(w, dt):
    lib = _lib.lib()
    co, ci, k, _ = w.shape
    wp = torch.empty(lib.sr_conv16_packed_weight_bytes(co, ci, k), dtype=torch.uint8, device=DEV)
    _lib.check(lib.sr_conv16_pack_weights(_lib.ptr(w.float().contiguous()), co, ci, k, IO[dt], _lib.ptr(wp),
                                          _lib.stream_ptr(w.device)), "sr_conv16_pack_weights")
    return wp


def _conv16_rc(x, wp, bias, res, out, co, k, stride, slope, io=None, out_dtype=None):
    """The raw return code of sr_conv16_nhwc_fwd on channels-last views."""
    b, ci, h, w = x.shape
    io = IO[x.dtype] if io is None else io
    out_dtype = (0 if out.dtype == torch.float32 else io) if out_dtype is None else out_dtype
    rsb, rsp = ops._strides(res) if res is not None else (0, 0)
    return _lib.lib().sr_conv16_nhwc_fwd(_lib.ptr(x), *ops._strides(x), _lib.ptr(wp), _lib.ptr(bias), _lib.ptr(res), rsb, rsp,
                                         _lib.ptr(out), *ops._strides(out), b, h, w, ci, co, k, stride,
                                         C.c_float(-1.0 if slope is None else slope), io, out_dtype, _lib.stream_ptr(x.device))


def _nhwc(t):
    return t.contiguous(memory_format=torch.channels_last)


def _sliced(t, dt, fill=None):
    """`t` ([B,C,H,W], CPU) as the channel slice [8, 8 + C) of a channels-last device tensor 16 channels wider (16-byte aligned
    rows), and that wider tensor."""
    b, c, h, w = t.shape
    wide = torch.full((b, c + 16, h, w), 7.0 if fill is None else fill, dtype=dt, device=DEV)
    wide = _nhwc(wide)
    view = wide[:, 8:8 + c]
    if fill is None:
        view.copy_(t.to(DEV).to(dt))
    return view, wide


def _idx(*shape):
    return torch.meshgrid(*[torch.arange(n, dtype=torch.int64) for n in shape], indexing="ij")


@functools.lru_cache(maxsize=None)
def _integer_case(shape, k, stride, small):
    """Integer operands (fp64, CPU) and their exact convolution sum.  small: every value in {-1, 0, 1}."""
    B, ci, H, W, co = shape
    b, c, y, x = _idx(B, ci, H, W)
    o, i, kh, kw = _idx(co, ci, k, k)
    xs = (7 * b + 3 * y + 5 * x + c) % 7 - 3
    ws = (5 * o + 3 * i + 2 * kh + kw) % 5 - 2
    if small:
        xs, ws = (7 * b + 3 * y + 5 * x + c) % 3 - 1, (5 * o + 3 * i + 2 * kh + kw) % 3 - 1
    xs, ws = xs.double(), ws.double()
    s = F.conv2d(xs, ws, None, stride=stride, padding=k // 2)
    rb, rc, ry, rx = _idx(*s.shape)
    res = ((rb + 2 * ry + rx + 3 * rc) % 5 - 2).double()
    bias = ((torch.arange(co) * 3) % 5 - 2).double()
    return xs, ws, bias, res, s


def _act(v, slope):
    return v if slope is None else F.leaky_relu(v, slope)


@pytest.mark.parametrize("slope", [None, 0.0, 0.5])
@pytest.mark.parametrize("k,stride", FORMS)
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("dt", DTYPES)
def test_exact_integers_bit_for_bit_fp32_output(dt, shape, k, stride, slope):
    """|sum| <= 9 * 64 * 6 << 2^24: every product and partial sum is exact whatever the order, so the fp32 output must EQUAL
    the fp64 convolution.  Input and output are channel slices of wider tensors whose other channels hold 7 and stay 7."""
    xs, ws, bias, res, s = _integer_case(shape, k, stride, False)
    co = shape[4]
    x, _ = _sliced(xs, dt)
    r = _nhwc(res.to(DEV).to(dt))
    out, wide = _sliced(s, torch.float32, fill=7.0)
    with torch.inference_mode():
        _lib.check(_conv16_rc(x, _pack(ws.to(DEV), dt), bias.float().to(DEV), r, out, co, k, stride, slope), "sr_conv16_nhwc_fwd")
    expect = _act(s + bias.view(1, -1, 1, 1) + res, slope).float()
    assert bool((wide[:, :8] == 7).all()) and bool((wide[:, 8 + co:] == 7).all())
    assert torch.equal(out.cpu(), expect), float((out.cpu() - expect).abs().max())


@pytest.mark.parametrize("slope", [None, 0.0, 0.5])
@pytest.mark.parametrize("k,stride", FORMS)
@pytest.mark.parametrize("shape", [(1, 8, 5, 7, 8), (3, 8, 17, 23, 40)])
@pytest.mark.parametrize("dt", DTYPES)
def test_exact_integers_bit_for_bit_16bit_output(dt, shape, k, stride, slope):
    """Ci = 8 with operands in {-1, 0, 1}: |sum + bias + residual| <= 76, and half of it, are exact in fp16 AND bf16 (8
    significant bits), so the rounded 16-bit output equals the fp64 result too.  Without bias / residual in one form."""
    xs, ws, bias, res, s = _integer_case(shape, k, stride, True)
    co = shape[4]
    x, _ = _sliced(xs, dt)
    with_extras = slope != 0.0
    r = _nhwc(res.to(DEV).to(dt)) if with_extras else None
    out, wide = _sliced(s, dt, fill=7.0)
    with torch.inference_mode():
        _lib.check(_conv16_rc(x, _pack(ws.to(DEV), dt), bias.float().to(DEV) if with_extras else None, r, out, co, k, stride, slope),
                   "sr_conv16_nhwc_fwd")
    expect = _act(s + bias.view(1, -1, 1, 1) + res if with_extras else s, slope)
    assert float(expect.abs().max()) <= 76
    assert bool((wide[:, :8] == 7).all()) and bool((wide[:, 8 + co:] == 7).all())
    assert torch.equal(out.cpu().double(), expect), float((out.cpu().double() - expect).abs().max())


def test_pack_rounds_like_tensor_to():
    """sr_conv16_pack_weights rounds to nearest even exactly as tensor.to(dtype) (ties, fp16 overflow -> inf, subnormals): the
    packed record of (tile 0, tap 0, step 0, lane r) starts with W[r][0]."""
    vals = torch.tensor([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 65519.9, 65520.0, 1e5, -1e5,
                         2.0 ** -25, 3 * 2.0 ** -25, 1e-40, -0.0, 0.1, -3.14159, 6.1e-5, 2.0 ** -24], dtype=torch.float32)
    w = torch.zeros((16, 8, 1, 1))
    w[:, 0, 0, 0] = vals
    for dt in DTYPES:
        wp = _pack(w.to(DEV), dt).cpu().view(torch.int16).view(-1, 8)          # [lane][8 values]
        got = wp[:16, 0]
        assert torch.equal(got, vals.to(dt).view(torch.int16)), dt
        assert not wp[16:32].any() and not wp[:16, 1:].any()                   # rows past Cout, other channels: zero


def _random_case(shape, k, stride, dt, seed, with_res, slope):
    B, ci, H, W, co = shape
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, ci, H, W), generator=g).to(dt)
    w = (torch.randn((co, ci, k, k), generator=g) * (1.0 / (k * k * ci) ** 0.5)).to(dt)       # |R| ~ 1: far from 65504
    bias = torch.randn((co,), generator=g)
    ho, wo = (H + 2 * (k // 2) - k) // stride + 1, (W + 2 * (k // 2) - k) // stride + 1
    res = torch.randn((B, co, ho, wo), generator=g).to(dt) if with_res else None
    return x, w, bias, res


def _check_bound(out, x, w, bias, res, k, stride, slope, u, tiny):
    """|out - R| <= u |R| + (K + 4) 2^-23 (A + |bias| + |residual|) + tiny, elementwise: R the fp64 result on the rounded
    operands, A the fp64 convolution of |w| with |x|, K = k^2 Ci -- one output rounding (u) plus fp32 accumulation of K
    products, bias and residual in any order."""
    xd, wd = x.double(), w.double()
    pre = F.conv2d(xd, wd, bias.double(), stride=stride, padding=k // 2)
    A = F.conv2d(xd.abs(), wd.abs(), bias.double().abs(), stride=stride, padding=k // 2)
    if res is not None:
        pre, A = pre + res.double(), A + res.double().abs()
    R = _act(pre, slope)
    K = k * k * x.shape[1]
    bound = u * R.abs() + (K + 4) * 2.0 ** -23 * A + tiny
    err = (out.cpu().double() - R).abs()
    worst = float((err / bound).max())
    print(f"conv16 bound: max err {float(err.max()):.3e}, worst err / bound {worst:.3f}, max |R| {float(R.abs().max()):.2f}")
    assert float(R.abs().max()) < 1000 and worst <= 1.0, worst


_U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
_TINY = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133, torch.float32: 2.0 ** -149}


@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("shape,k,stride", [(sh, k, s) for sh in SHAPES for k, s in FORMS] + [((1, 64, 120, 160, 64), 3, 1)])
@pytest.mark.parametrize("dt", DTYPES)
def test_random_data_within_the_derived_bound(dt, shape, k, stride, out_f32):
    with_res, slope = shape[1] != 24, (0.2 if shape[4] != 64 else None)
    x, w, bias, res = _random_case(shape, k, stride, dt, 11 * shape[1] + shape[4] + k + stride, with_res, slope)
    xd, _ = _sliced(x, dt)
    rd = _nhwc(res.to(DEV)) if res is not None else None
    odt = torch.float32 if out_f32 else dt
    ho, wo = (shape[2] + 2 * (k // 2) - k) // stride + 1, (shape[3] + 2 * (k // 2) - k) // stride + 1
    out = _nhwc(torch.empty((shape[0], shape[4], ho, wo), dtype=odt, device=DEV))
    with torch.inference_mode():
        _lib.check(_conv16_rc(xd, _pack(w.to(DEV), dt), bias.to(DEV), rd, out, shape[4], k, stride, slope), "sr_conv16_nhwc_fwd")
    _check_bound(out.float(), x, w, bias, res, k, stride, slope, 0.0 if out_f32 else _U[dt], _TINY[odt])


@pytest.mark.parametrize("dt", DTYPES)
def test_pointwise_with_a_batch_stride_past_2_to_31(dt):
    """(2, 256, 15, 20, 128) 1x1 with the second image 2^31 + 8 elements behind the first: image offsets are 64-bit."""
    shape, k, stride = (2, 256, 15, 20, 128), 1, 1
    x, w, bias, res = _random_case(shape, k, stride, dt, 5, True, 0.2)
    B, ci, H, W, co = shape
    sb = 2 ** 31 + 8
    store = torch.empty(sb + H * W * ci, dtype=dt, device=DEV)                 # (4 GiB, untouched but for the two images)
    xd = store.as_strided((B, ci, H, W), (sb, 1, W * ci, ci))
    xd.copy_(x.to(DEV))
    out = _nhwc(torch.empty((B, co, H, W), dtype=dt, device=DEV))
    with torch.inference_mode():
        _lib.check(_conv16_rc(xd, _pack(w.to(DEV), dt), bias.to(DEV), _nhwc(res.to(DEV)), out, co, k, stride, 0.2), "sr_conv16_nhwc_fwd")
    _check_bound(out.float(), x, w, bias, res, k, stride, 0.2, _U[dt], _TINY[dt])


@pytest.mark.parametrize("k,stride", FORMS)
@pytest.mark.parametrize("dt", DTYPES)
def test_two_launches_give_the_same_bits(dt, k, stride):
    shape = (2, 64, 33, 64, 160)
    x, w, bias, res = _random_case(shape, k, stride, dt, 3, True, 0.2)
    xd, wp, rd = _nhwc(x.to(DEV)), _pack(w.to(DEV), dt), _nhwc(res.to(DEV))
    outs = []
    with torch.inference_mode():
        for _ in range(2):
            out = _nhwc(torch.zeros(res.shape, dtype=dt, device=DEV))
            _lib.check(_conv16_rc(xd, wp, bias.to(DEV), rd, out, shape[4], k, stride, 0.2), "sr_conv16_nhwc_fwd")
            outs.append(out)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    assert bool(torch.isfinite(outs[0]).all()) and float(outs[0].float().abs().max()) > 0


def test_refusals_launch_nothing():
    dt = torch.bfloat16
    B, ci, H, W, co = 1, 16, 6, 9, 16
    wide = _nhwc(torch.randn((B, ci + 16, H, W), device=DEV).to(dt))
    x = wide[:, 8:8 + ci]
    wp = _pack(torch.randn((co, ci, 3, 3), device=DEV), dt)
    wp1 = _pack(torch.randn((co, ci, 1, 1), device=DEV), dt)
    out_wide = _nhwc(torch.full((B, co + 16, H, W), 7.0, dtype=dt, device=DEV))
    out = out_wide[:, 8:8 + co]
    res = _nhwc(torch.randn((B, co, H, W), device=DEV).to(dt))
    odd = _nhwc(torch.randn((B, ci + 4, H, W), device=DEV).to(dt))              # pixel stride 20: not a multiple of 8
    cases = [
        (_conv16_rc(wide[:, 4:4 + ci], wp, None, None, out, co, 3, 1, None), SR_ERR_UNSUPPORTED),        # rows 8 bytes off
        (_conv16_rc(odd[:, :ci], wp, None, None, out, co, 3, 1, None), SR_ERR_UNSUPPORTED),              # stride % 8 != 0
        (_conv16_rc(x, wp, None, None, out_wide[:, 4:4 + co], co, 3, 1, None), SR_ERR_UNSUPPORTED),
        (_conv16_rc(x, wp, None, odd[:, 4:4 + co], out, co, 3, 1, None), SR_ERR_UNSUPPORTED),            # residual likewise
        (_conv16_rc(wide[:, :12], wp, None, None, out, co, 3, 1, None), SR_ERR_UNSUPPORTED),             # Cin = 12
        (_conv16_rc(x, wp, None, None, out_wide[:, 8:20], 12, 3, 1, None), SR_ERR_UNSUPPORTED),          # Cout = 12
        (_conv16_rc(x, wp, None, res, out, co, 3, 1, -2.0), SR_ERR_UNSUPPORTED),                         # SiLU
        (_conv16_rc(x, wp, None, res, out, co, 3, 1, None, io=3), SR_ERR_INVALID_ARGUMENT),
        (_conv16_rc(x, wp, None, res, out, co, 3, 1, None, io=0), SR_ERR_INVALID_ARGUMENT),
        (_conv16_rc(x, wp, None, res, out, co, 3, 1, None, out_dtype=1), SR_ERR_INVALID_ARGUMENT),       # bf16 in, fp16 out
        (_conv16_rc(x, wp, None, res, out, co, 5, 1, None), SR_ERR_INVALID_ARGUMENT),
        (_conv16_rc(x, wp, None, res, out, co, 3, 3, None), SR_ERR_INVALID_ARGUMENT),
        (_conv16_rc(x, wp1, None, res, out, co, 1, 2, None), SR_ERR_INVALID_ARGUMENT),
    ]
    torch.cuda.synchronize()
    assert [got for got, _ in cases] == [want for _, want in cases]
    assert bool((out_wide == 7).all())
    _lib.check(_conv16_rc(x, wp, None, res, out, co, 3, 1, None), "sr_conv16_nhwc_fwd")                  # (the accepted call does write)
    assert not bool((out == 7).all()) and bool((out_wide[:, :8] == 7).all()) and bool((out_wide[:, 8 + co:] == 7).all())


@pytest.mark.parametrize("dt", DTYPES)
def test_conv_stack_trains_on_the_16bit_mfma_kernel(dt, monkeypatch):
    """The conv stack of test_gpu_half_io.py (same modules, seeds, sizes) under torch.autocast with
    experimental.autocast_mfma16(mode=2): every layer sr_conv16_supported accepts runs its forward AND its data gradient on
    sr_conv16_nhwc_fwd; outputs and parameter gradients agree with the fp32 run within that test's tolerances for 16-bit
    activations over ~20 layers (3e-2 fp16, 2e-1 bf16).  fp16: the loss is scaled by 2^10 and the gradients divided back, as
    a loss scaler does -- the data gradient now travels in fp16 and underflows by design otherwise (the reference's precision-16
    training runs under a scaler too)."""
    before = (autograd_ops.HALF_IO, autograd_ops.MFMA16, autograd_ops.STORE_HALF)
    torch.manual_seed(0)
    enc = synthetic.seeded_fill_(CVEncoder(16, [8, 12, 16, 24], [16, 24, 32, 48]), seed=1).to(DEV)
    dec = synthetic.seeded_fill_(DepthDecoderPP([6] + enc.num_ch_enc), seed=2).to(DEV)
    g = torch.Generator().manual_seed(5)
    B, H, W = 2, 32, 48
    vol = torch.randn((B, 16, H, W), generator=g).to(DEV).requires_grad_(True)
    pyr = [torch.randn((B, c, H >> i, W >> i), generator=g).to(DEV) for i, c in enumerate([8, 12, 16, 24])]
    f0 = torch.randn((B, 6, 2 * H, 2 * W), generator=g).to(DEV)
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
        n_fwd = sum(name == "sr_conv16_nhwc_fwd" for name, _ in calls)
        (loss * s).backward()
        grads = {n: p.grad / s for m in (enc, dec) for n, p in m.named_parameters() if p.grad is not None}
        return out, grads, vol.grad / s, n_fwd

    ref_out, ref_g, ref_dv, n0 = step(False)
    assert n0 == 0 and not any(name.startswith("sr_conv16") for name, _ in calls)        # fp32: the new code is not reached
    calls.clear()
    with experimental.autocast_mfma16(mode=2):
        out, gr, dv, n_fwd = step(True)
    assert (autograd_ops.HALF_IO, autograd_ops.MFMA16, autograd_ops.STORE_HALF) == before
    n_all = sum(name == "sr_conv16_nhwc_fwd" for name, _ in calls)
    assert n_fwd > 0 and n_all - n_fwd > 0, (n_fwd, n_all)                                 # forward, and backward
    # no layer the new kernel supports went to a Winograd or pointwise 16-bit-I/O kernel
    sup = _lib.lib().sr_conv16_supported
    for name, a in calls:
        if name == "sr_conv3x3_wino_io_nhwc_fwd":
            assert not sup(a[11], a[12], a[13], a[14], a[15], 3, 1), a[11:16]
        if name == "sr_pw_conv_io_nhwc_fwd":
            assert not sup(a[11], a[12], 1, a[13], a[14], 1, 1), a[11:15]
    tol = 3e-2 if dt == torch.float16 else 2e-1
    for i in range(4):
        k = f"log_depth_pred_s{i}_b1hw"
        assert out[k].dtype == dt and torch.isfinite(out[k]).all()
        assert rel_err(out[k].float(), ref_out[k]) < tol, (k, rel_err(out[k].float(), ref_out[k]))
    assert sorted(gr) == sorted(ref_g) and dv.dtype == torch.float32 and torch.isfinite(dv).all()
    assert all(torch.isfinite(v).all() for v in gr.values())

    def l2(a, b):
        return float((a.float() - b).norm() / b.norm().clamp_min(1e-12))
    errs = [l2(gr[n], ref_g[n]) for n in gr]
    print(f"conv16 stack {dt}: median grad err {np.median(errs):.3e}, max {max(errs):.3e}, conv16 launches fwd {n_fwd} bwd {n_all - n_fwd}")
    assert np.median(errs) < tol, (np.median(errs), max(errs))
