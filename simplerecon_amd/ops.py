"""Host-side plumbing for the HIP conv stack: channels-last tensor views, packed-weight cache,
and thin wrappers that hand raw pointers/strides to the C ABI (include/simplerecon_hip.h).

A "channels-last view" is a logically [B,C,H,W] torch tensor whose memory is [B,H,W,Ctot] with
this tensor occupying channels [c0, c0+C) of each pixel -- either a dense channels_last tensor or
a channel slice `buf[:, c0:c1]` of one.  Kernels take (pointer, batch stride, pixel stride)."""
import contextlib
import os
import weakref

import torch
from torch import nn

from . import _lib

# When set to a list, every timed launch (_timed) appends (kernel symbol, algorithmic FLOPs, start event, end event, shape,
# executed FLOPs): bench.py uses it to time the dominant kernel with HIP events on the launch stream.  The symbol and the
# executed FLOPs are reported by the launcher that issued the kernel (sr_last_launch), not worked out again here.
PROFILE = None

# Packed weights (and the other tensors derived from a module's parameters), per module: {cache tag: [state key, payload,
# pack fence]}.  They are produced on whichever stream made the first call; a consumer on ANOTHER stream (the sub-batch
# streams of DepthModel.hot_path, the image-prior side stream) must not start before that work finished.  The fence is
# (event recorded behind the pack, its stream handle, device), or None once the event has completed.
_PACKED = weakref.WeakKeyDictionary()
_NO_ENTRIES = {}   # (read only: what a module without entries looks up)
# The state key of an entry is (version counter, address) of every tensor the payload is derived from (_state_key).  It sees
# what bumps a version counter: in-place updates under no_grad (optimizer steps), load_state_dict, nn.init.*, writes through
# detach(), and a parameter replaced by a new tensor (module.to(...), assignment).  It does NOT see writes through `.data`
# (`w.data.mul_()`, `w.data.copy_()` leave `w._version` unchanged): whoever writes that way calls forget_packed(module).
# Nor does it see a kernel that writes a parameter through its raw address.  optim.AdamW does exactly that, so its step() bumps
# the counter itself (torch.autograd.graph.increment_version) for every parameter that had a gradient, also when the device
# skips the step on a found-inf flag the host cannot see: the entry is then packed again from unchanged weights, which costs
# time and changes nothing.  Any other code that updates weights from a kernel owes the cache the same call.
_FORGET_EPOCH = 0   # bumped by forget_packed: a captured HIP graph (graph.GraphedCallable) refuses to replay across it


def _cached(mod, tag, key, build, *args):
    """build(*args), cached as `mod`'s `tag` entry until `key` (its _state_key and anything else the payload depends on)
    changes.  Runs once per launch: a hit is one lookup and one key comparison."""
    e = _PACKED.get(mod, _NO_ENTRIES).get(tag)
    if e is not None and e[0] == key:
        if e[2] is not None:
            _await_pack(e)
        return e[1]
    payload = build(*args)
    fence = None
    # weights are packed during warm-up, never inside a capture (graph.GraphedCallable warms up first)
    if _lib.cuda_available() and not _lib.capturing():
        device = mod.weight.device
        st = torch.cuda.current_stream(device)
        ev = torch.cuda.Event()
        ev.record(st)
        fence = (ev, st.cuda_stream, device)
    _PACKED.setdefault(mod, {})[tag] = [key, payload, fence]
    return payload


def forget_packed(module):
    """Drops every cached payload (packed weights, folded biases) of `module` and its submodules, so that the next call packs
    again from the current parameters.  For code that writes parameters through `.data`, which the cache key cannot see; a
    HIP graph captured before the call bakes the old payloads in and refuses to replay afterwards (capture again)."""
    global _FORGET_EPOCH
    for m in module.modules():
        _PACKED.pop(m, None)
    _FORGET_EPOCH += 1


def packed_payloads(modules=None):
    """The payloads currently cached for `modules` (roots; their submodules included) -- for every module when None.  A
    captured HIP graph holds on to them: it bakes their addresses in, while a later eager call that re-packs drops them."""
    if modules is None:
        entries = list(_PACKED.values())
    else:
        entries = [_PACKED[m] for root in modules for m in root.modules() if m in _PACKED]
    return [e[1] for entry in entries for e in entry.values()]


def _await_pack(e):
    if _lib.capturing():
        return
    ev, stream, device = e[2]
    if ev.query():
        e[2] = None
        return
    st = torch.cuda.current_stream(device)
    if st.cuda_stream != stream:
        st.wait_event(ev)


# the leading weight dimensions the library's sr_<kind>_packed_weight_floats / sr_<kind>_pack_weights take
_PACK_DIMS = {"conv": 3, "wino": 2, "wino4": 2, "stem": 1, "conv3x3_c16": 2}


def _pack(kind, w, *fmt):
    """The library's `kind` packing of the contiguous fp32 weight `w` ([Co, Ci, k, k]) into a new tensor (uncached).  `fmt`:
    what the pack call takes behind the dimensions ("wino": the split format, which the launch is handed too)."""
    dims = w.shape[:_PACK_DIMS[kind]]
    packed = torch.empty(getattr(_lib.lib(), f"sr_{kind}_packed_weight_floats")(*dims), dtype=torch.float32, device=w.device)
    _lib.call(f"sr_{kind}_pack_weights", w.device, w, *dims, *fmt, packed)
    return packed


def empty_nhwc(b, c, h, w, device):
    return torch.empty((b, c, h, w), dtype=torch.float32, device=device, memory_format=torch.channels_last)


def conv_out_hw(h, w, stride, ksize=3):
    pad = ksize // 2
    return (h + 2 * pad - ksize) // stride + 1, (w + 2 * pad - ksize) // stride + 1


def tf_same_pads(h, w, ksize, stride):
    """(top, left, bottom, right) zero padding of a TensorFlow-"SAME" convolution: output size ceil(i / stride),
    the odd pixel of padding goes below / right (what timm's Conv2dSame computes per call for its tf_* models)."""
    def one(i):
        total = max((-(-i // stride) - 1) * stride + ksize - i, 0)
        return total // 2, total - total // 2
    (pt, pb), (pl, pr) = one(h), one(w)
    return pt, pl, pb, pr


def _act_code(leaky, act):
    """The activation code the C ABI carries in `leaky_slope` (include/simplerecon_hip.h)."""
    if act is None:
        return -1.0 if leaky is None else float(leaky)
    if leaky is not None:
        raise ValueError("pass either `leaky` or `act`, not both")
    if act == "silu":
        return -2.0
    raise ValueError(f"unknown activation {act!r}")


def _is_nhwc_view(t):
    if t.dim() != 4:
        return False
    b, c, h, w = t.shape
    sb, sc, sh, sw = t.stride()
    if c == 1:
        sc = 1
    return sc == 1 and sw >= c and sh == w * sw and (b == 1 or sb >= h * sh)


def as_nhwc(t, name="tensor"):
    """Returns `t` if it already is a channels-last view, else a dense channels_last repack."""
    _lib.require_device_f32(name, t)
    if t.dim() != 4:
        raise ValueError(f"{name} must be [B,C,H,W], got {tuple(t.shape)}")
    if _is_nhwc_view(t):
        return t
    return t.contiguous(memory_format=torch.channels_last)


def _strides(t):
    """(batch stride, pixel stride) in elements of a channels-last view."""
    b, c, h, w = t.shape
    sb, _, _, sw = t.stride()
    if b == 1:
        sb = h * w * sw
    return sb, sw


def _state_key(conv, bn):
    # (version, address) of every tensor the packed weight is derived from; read through the modules' own dictionaries
    # (nn.Module.__getattr__ is a slow path and this runs once per launch)
    p = conv._parameters
    w, b = p["weight"], p.get("bias")
    if bn is None:
        if b is None:
            return (w._version, w.data_ptr())
        return (w._version, w.data_ptr(), b._version, b.data_ptr())
    ts = [w] if b is None else [w, b]
    bufs, bp = bn._buffers, bn._parameters
    ts += [bufs["running_mean"], bufs["running_var"]]
    if bn.affine:
        ts += [bp["weight"], bp["bias"]]
    return tuple((t._version, t.data_ptr()) if t is not None else None for t in ts)


def bn_affine(bn):
    """Eval-mode BatchNorm2d as the per-channel affine ATen's inference path applies:
    scale = weight / sqrt(running_var + eps), shift = bias - running_mean * scale."""
    if bn.running_mean is None or bn.running_var is None:
        raise _lib.HipLibraryError("BatchNorm without running statistics cannot run in inference mode")
    scale = torch.rsqrt(bn.running_var.detach() + bn.eps)
    if bn.affine:
        scale = scale * bn.weight.detach()
    shift = -bn.running_mean.detach() * scale
    if bn.affine:
        shift = shift + bn.bias.detach()
    return scale.contiguous(), shift.contiguous()


def _effective_weight(conv, bn):
    """(weight, bias) of `conv` with an eval-mode BatchNorm `bn` behind it folded in (one-off, at pack time)."""
    w = conv.weight.detach()
    b = conv.bias.detach() if conv.bias is not None else None
    if bn is not None:
        scale, shift = bn_affine(bn)
        w = w * scale.view(-1, 1, 1, 1)
        b = shift if b is None else b * scale + shift
    return w.contiguous(), b


def _check_conv(conv):
    k = conv.kernel_size[0]
    if conv.kernel_size[0] != conv.kernel_size[1] or k not in (1, 3) or conv.groups != 1 \
            or conv.dilation != (1, 1) or tuple(conv.padding) != (k // 2,) * 2 \
            or conv.padding_mode not in ("zeros", "replicate"):
        raise _lib.HipLibraryError(f"unsupported Conv2d configuration for the HIP path: {conv}")


def _pack_folded(kind, conv, bn, *fmt):
    """(the `kind` packing (_pack) of conv's weight with `bn` folded in, bias)."""
    _lib.require_device_f32("conv weight", conv.weight)
    _check_conv(conv)
    w, bias = _effective_weight(conv, bn)
    return _pack(kind, w, *fmt), bias


def packed_weight(conv: nn.Conv2d, bn=None):
    """(packed weight, bias) for the direct kernel; cached until a parameter changes."""
    return _cached(conv, "direct", _state_key(conv, bn), _pack_folded, "conv", conv, bn)


# 1x1 / stride-1 convolutions run on the hand-written pointwise MFMA GEMM of csrc/sr_pw.hip (deterministic, r04); False sends
# the ungated ones to the implicit-GEMM conv kernel (the reference path of the tests)
USE_PW_1X1 = True
# which of the two pointwise kernels: "auto" = the LDS-tiled one for batch-dense maps of at least PW_TILED_MIN_ROWS pixels
# (the HBM-bound full-resolution skips: 168 vs 182 us for 192 -> 64 @ 8x240x320), the direct one below that -- on the small-M
# encoder GEMMs the tiled kernel's one or two workgroups per CU cannot hide their load latency and it measured no faster
# (38 vs 36 us for 1536 -> 256 @ 8x15x20, profiles/r04_pw_plan_sweep.txt); "1" / "0" force one of them
PW_TILED = os.environ.get("SR_PW_TILED", "auto")
PW_TILED_MIN_ROWS = 100000


def _pack_linear(lin):
    return _pack("conv", lin.weight.detach().reshape(lin.out_features, lin.in_features, 1, 1).contiguous())


def linear(x, lin: nn.Linear, leaky=None):
    """act(x @ W^T + b) over the last dimension through the 1x1 instantiation of the HIP conv kernel
    ([M, Cin] row-major IS a 1 x M channels-last image).  Used by networks.MLP.forward."""
    _lib.require_device_f32("linear input", x)
    _lib.refuse_autograd(x, lin.weight)
    cin, cout = lin.in_features, lin.out_features
    if x.shape[-1] != cin:
        raise ValueError(f"linear expects {cin} input features, got {x.shape[-1]}")
    x2 = x.reshape(-1, cin).contiguous()
    m = x2.shape[0]
    out = torch.empty((m, cout), dtype=torch.float32, device=x.device)
    if m == 0:
        return out.view(*x.shape[:-1], cout)
    wp = _cached(lin, "linear", _state_key(lin, None), _pack_linear, lin)
    bias = lin.bias.detach() if lin.bias is not None else None
    _lib.call("sr_conv2d_nhwc_fwd", x.device, x2, m * cin, cin, wp, bias, None, 0, 0, out, m * cout, cout, 1, 1, m, cin, cout,
              1, 1, -1.0 if leaky is None else float(leaky))
    return out.view(*x.shape[:-1], cout)


def wino_split_mode():
    """'' (off: fp32 MFMA, the product path), 'bf16' or 'f16': the fenced split-precision Winograd variant -- the library's
    option SR_WINO_SPLIT (set with _lib.set_option / experimental.split_precision), which a call reads once (`split`)."""
    return _lib.split_mode_name("SR_WINO_SPLIT")


def packed_wino_weight(conv: nn.Conv2d, bn=None, split=None):
    """(Winograd-packed weight U = G g G^T, bias); cached until a parameter or the format changes.  `split`: the format, 0 /
    1 / 2 = fp32 / bf16 pieces / f16 pieces (None: what SR_WINO_SPLIT says now) -- the launch on this weight takes the same."""
    split = _lib.get_option("SR_WINO_SPLIT") if split is None else split
    return _cached(conv, "wino", (_state_key(conv, bn), split), _pack_folded, "wino", conv, bn, split)


# Which 3x3 / stride-1 layers take the F(4x4, 3x3) kernel (csrc/sr_wino4.hip): "1" (default) = the library's rule
# (sr_conv_prefers_wino4: the full-resolution layers at batch 8), "0" = none, "2" = every layer it applies to (tests).
# Read once, handed to the library as an argument.
WINO4_MODE = int(os.environ.get("SR_CONV_WINO4", "1"))
# kernel form: 0 = the library's default, 1 = two independent 4-wave workgroups per CU, 2 = the 8-wave ping-pong workgroup
# (bit-identical results; A/B measurements)
WINO4_VARIANT = int(os.environ.get("SR_WINO4_VARIANT", "0"))


def packed_wino4_weight(conv: nn.Conv2d, bn=None):
    """(F(4x4, 3x3)-packed weight U = G g G^T, bias); cached until a parameter changes."""
    return _cached(conv, "wino4", _state_key(conv, bn), _pack_folded, "wino4", conv, bn)


# Pure functions of the layer shape inside the C library (launch-plan choices): asked once per shape, not once per launch.
_SHAPE_QUERIES = {}


def _drop_shape_queries(*_):
    _SHAPE_QUERIES.clear()


# launch plans depend on the forcing switches (SR_PT_*, SR_PW_*, SR_CONV_WINO ...): any option change drops the cached answers
_lib.OPTION_LISTENERS.append(_drop_shape_queries)


def _shape_query(lib, name, *shape, dev=None):
    # `dev`: device index of the tensors (the answers may depend on the device's CU count: sr_conv_prefers_wino4, split-K plans)
    key = (name, shape, dev)
    v = _SHAPE_QUERIES.get(key)
    if v is None:
        v = _SHAPE_QUERIES[key] = getattr(lib, name)(*shape)
    return v


def conv2d(x, conv: nn.Conv2d, residual=None, leaky=None, out=None, bn=None, act=None, tf_same=False, gate=None):
    """act(bn(conv(x) + bias) [+ residual]) with nn.Conv2d semantics (zero or replicate padding); `bn` is an eval-mode
    BatchNorm2d folded into weight and bias.  `leaky` = LeakyReLU slope, or act="silu".  tf_same=True replaces the module's
    symmetric padding by TensorFlow-"SAME" padding (tf_same_pads).  Batch-size invariance: every kernel on the default path is
    run-to-run deterministic, but the RESULT OF A FRAME MAY DEPEND ON THE BATCH IT IS IN (and on the CU count of the device) in
    its low-order bits: the launch plans are chosen from the total number of work items, B included -- a 3x3 / stride-1 layer
    runs F(4x4) Winograd at one batch size and F(2x2) at another (sr_conv_prefers_wino4: 64 -> 64 at 240x320 is F(2x2) at B = 1,
    F(4x4) at B = 8; error constants 3e-7 vs 1.3e-6 of the output range), and the Winograd / direct / pointwise plans split K on
    small maps.  Within ONE plan the per-pixel arithmetic does not depend on B.  tests/test_gpu_determinism.py pins the
    run-to-run statement and the 1x1 cases, tests/test_gpu_e2e_full_size.py::test_batch_1_and_batch_8_agree_frame_by_frame the
    model-level agreement (to the element-wise tolerance each holds against the oracle, not bitwise).  `gate` ([B, Cin], 1x1 /
    stride-1 convs only): the input is scaled per image and input channel while it is loaded (the squeeze-excite gate of an
    MBConv block).  Returns a channels-last view."""
    _lib.refuse_autograd(x, conv.weight)
    x = as_nhwc(x, "conv input")
    b, ci, h, w = x.shape
    if ci != conv.in_channels:
        raise ValueError(f"conv expects {conv.in_channels} input channels, got {ci}")
    k, s = conv.kernel_size[0], conv.stride[0]
    if conv.stride[0] != conv.stride[1] or s not in (1, 2):
        raise _lib.HipLibraryError(f"unsupported stride {conv.stride}")
    pads = tf_same_pads(h, w, k, s) if tf_same else (k // 2,) * 4
    ho, wo = (h + pads[0] + pads[2] - k) // s + 1, (w + pads[1] + pads[3] - k) // s + 1
    co = conv.out_channels
    if out is None:
        out = empty_nhwc(b, co, ho, wo, x.device)
    else:
        if tuple(out.shape) != (b, co, ho, wo) or not _is_nhwc_view(out):
            raise ValueError(f"`out` must be a channels-last view of shape {(b, co, ho, wo)}")
        _lib.require_device_f32("out", out)
    lib = _lib.lib()
    replicate = conv.padding_mode == "replicate"
    padded = pads != (k // 2,) * 4
    if padded and replicate:
        raise _lib.HipLibraryError("explicit padding is implemented for zero padding only")
    use_wino = (not replicate) and (not padded) and bool(_shape_query(lib, "sr_conv_prefers_wino", b, h, w, ci, co, k, s, dev=x.device.index))
    if residual is not None:
        residual = as_nhwc(residual, "residual")
        if tuple(residual.shape) != (b, co, ho, wo):
            raise ValueError(f"residual shape {tuple(residual.shape)} != output shape {(b, co, ho, wo)}")
    if b == 0:
        return out
    isb, isp = _strides(x)
    osb, osp = _strides(out)
    rsb, rsp = _strides(residual) if residual is not None else (0, 0)
    split = _lib.get_option("SR_WINO_SPLIT") if use_wino else 0   # read ONCE: the cache key, the pack's and the launch's format
    if split and not (ci % 4 == 0 and co % 4 == 0 and _aligned16(x, isb, isp) and _aligned16(out, osb, osp)
                      and _aligned16(residual, rsb, rsp)):
        # the fenced split-precision Winograd (SR_WINO_SPLIT, csrc/sr_wino_split.hip) has the vector instantiation only:
        # unaligned tensors and channel counts that are no multiple of 4 take the direct fp32 kernel instead
        use_wino, split = False, 0
    if gate is not None:
        _lib.require_device_f32("gate", gate)
        if k != 1 or s != 1 or tuple(gate.shape) != (b, ci) or not gate.is_contiguous():
            raise ValueError(f"`gate` needs a 1x1 / stride-1 conv and a contiguous [{b}, {ci}] tensor")
    slope = _act_code(leaky, act)
    strides = (isb, isp, osb, osp, rsb, rsp)
    if k == 1 and s == 1 and not padded and not replicate and (USE_PW_1X1 or gate is not None) and ci % 4 == 0 \
            and _aligned16(x, isb, isp):
        shape = (b, ci, h, w, co, k, s, ho, wo, residual is not None)
        if _conv_pointwise(lib, x, *packed_weight(conv, bn), residual, out, gate, strides, shape, slope) == 0:
            return out
        # SR_ERR_UNSUPPORTED (a per-image byte range past 2^31): the implicit-GEMM kernel below, whose addressing is 64-bit
    if gate is not None:
        raise _lib.HipLibraryError("a gated 1x1 convolution needs Cin % 4 == 0 and 16-byte aligned input rows")
    if k == 1 and s == 1 and (w % 32 != 0 or h % 4 != 0) and (isp, isb) == (ci, h * w * ci) \
            and (osp, osb) == (co, h * w * co) and (residual is None or (rsp, rsb) == (co, h * w * co)):
        # a 1x1 conv over dense channels-last maps is a [B*H*W, Cin] x [Cin, Cout] product: hand the kernel the
        # pixels as one 32- (or 8-) wide strip so that no output tile is cut at image borders (15x20 maps would
        # leave 37 % of every 4x32 tile empty).  Same per-pixel arithmetic, same result.
        m = b * h * w
        fw = 32 if m % 32 == 0 else 8 if m % 8 == 0 else 0
        if fw:
            b, h, w, ho, wo = 1, m // fw, fw, m // fw, fw
            strides = (m * ci, isp, m * co, osp, m * co if residual is not None else 0, rsp)
    shape = (b, ci, h, w, co, k, s, ho, wo, residual is not None)
    w4_form = _shape_query(lib, "sr_conv_prefers_wino4", b, h, w, ci, co, WINO4_MODE, dev=x.device.index) \
        if (use_wino and WINO4_MODE and not split) else 0   # 0: F(2x2); 1 / 3: the kernel form the rule picks
    if w4_form and _conv_wino4(lib, x, *packed_wino4_weight(conv, bn), residual, out, strides, shape, slope,
                               WINO4_VARIANT or w4_form) == 0:
        return out
    if use_wino:
        if _conv_wino(lib, x, *packed_wino_weight(conv, bn, split), residual, out, strides, shape, slope, split) == 0:
            return out
        # SR_ERR_UNSUPPORTED from the Winograd entry point (a per-image byte range past 2^31: its buffer descriptors carry 32-bit
        # offsets): the implicit-GEMM kernel serves the shape with 64-bit addressing, as it did before r04
        wp, bias = packed_weight(conv, bn)
        isb, isp, osb, osp, rsb, rsp = strides
        _lib.call("sr_conv2d_nhwc_fwd", x.device, x, isb, isp, wp, bias, residual, rsb, rsp, out, osb, osp, b, h, w, ci, co,
                  k, s, slope)
        return out
    _conv_direct(lib, x, *packed_weight(conv, bn), residual, out, strides, shape, slope, pads if padded else None, replicate)
    return out


def _aligned16(t, sb, sp):
    """None, or a channels-last view whose pixel rows all start 16-byte aligned (the kernels' vector instantiations)."""
    return t is None or (t.data_ptr() % 16 == 0 and sp % 4 == 0 and sb % 4 == 0)


def _timed(device, flops, shape, fn, *args, name=None):
    """fn(*args) on `device` -> the library's rc.  With PROFILE on, two timing events bracket the launch and a launch that
    succeeded appends (kernel name, algorithmic FLOPs, start event, end event, shape, executed FLOPs): `flops` and `shape`
    are facts of the call, the kernel's name and the FLOPs it executed are what the launcher noted (_lib.last_launch).  The
    MLP sweep alone passes `name` -- its entry point, sr_mlp_volume_fwd, which the benchmark keys on -- and is not asked."""
    prof = PROFILE
    with _lib.on_device(device):
        if prof is None:
            return fn(*args)
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ev0.record()
        rc = fn(*args)
        ev1.record()
        if rc == 0:
            name, executed = (name, None) if name is not None else _lib.last_launch()
            prof.append((name, flops, ev0, ev1, shape, executed))
    return rc


def _launch(x, shape, entry, fallback, fn, *args):
    """A conv launch through _timed; raises for any error but SR_ERR_UNSUPPORTED with a `fallback` behind it (`entry`: the
    call's name in the message)."""
    if PROFILE is None:   # (skips _timed's call frame: a quarter microsecond per launch on a host-bound batch-1 path)
        with _lib.on_device(x.device):
            rc = fn(*args)
    else:
        b, ci, h, w, co, k, s, ho, wo, _ = shape
        rc = _timed(x.device, 2.0 * b * ho * wo * co * ci * k * k, shape, fn, *args)
    if rc != 0 and (rc != _lib.ERR_UNSUPPORTED or not fallback):
        _lib.check(rc, entry)
    return rc


def _conv_pointwise(lib, x, wp, bias, residual, out, gate, strides, shape, slope):
    """1x1 / stride-1: the pointwise GEMM kernels of csrc/sr_pw.hip (the LDS-tiled one on large batch-dense maps)."""
    isb, isp, osb, osp, rsb, rsp = strides
    b, ci, h, w, co = shape[:5]
    m = b * h * w
    dense = b == 1 or (isb == h * w * isp and osb == h * w * osp and (residual is None or rsb == h * w * rsp))
    if dense and (PW_TILED == "1" or (PW_TILED == "auto" and m >= PW_TILED_MIN_ROWS)):
        nbytes = _shape_query(lib, "sr_pw_conv_tiled_workspace_bytes", m, ci, co, dev=x.device.index)
        ws = _workspace(x.device, "pw_splitk", nbytes) if nbytes else None
        return _launch(x, shape, "sr_pw_conv_tiled_nhwc_fwd", gate is None, lib.sr_pw_conv_tiled_nhwc_fwd,
                       _lib.ptr(x), isp, _lib.ptr(wp), _lib.ptr(bias), _lib.ptr(gate), _lib.ptr(residual), rsp, _lib.ptr(out),
                       osp, m, h * w, ci, co, slope, _lib.ptr(ws), nbytes, _lib.stream_ptr(x.device))
    return _launch(x, shape, "sr_pw_conv_nhwc_fwd", gate is None, lib.sr_pw_conv_nhwc_fwd, _lib.ptr(x), isb, isp,
                   _lib.ptr(wp), _lib.ptr(bias), _lib.ptr(gate), _lib.ptr(residual), rsb, rsp, _lib.ptr(out), osb, osp, b,
                   h * w, ci, co, slope, _lib.stream_ptr(x.device))


def _conv_wino4(lib, x, wp, bias, residual, out, strides, shape, slope, variant):
    """3x3 / stride 1: F(4x4, 3x3) Winograd (csrc/sr_wino4.hip) in kernel form `variant`; SR_ERR_UNSUPPORTED without
    launching when a tensor or the bias is not 16-byte aligned."""
    isb, isp, osb, osp, rsb, rsp = strides
    b, ci, h, w, co = shape[:5]
    if not (_aligned16(x, isb, isp) and _aligned16(out, osb, osp) and _aligned16(residual, rsb, rsp)
            and (bias is None or bias.data_ptr() % 16 == 0)):
        return _lib.ERR_UNSUPPORTED
    return _launch(x, shape, "sr_conv3x3_wino4_nhwc_fwd", True, lib.sr_conv3x3_wino4_variant_nhwc_fwd, _lib.ptr(x), isb, isp,
                   _lib.ptr(wp), _lib.ptr(bias), _lib.ptr(residual), rsb, rsp, _lib.ptr(out), osb, osp, b, h, w, ci, co,
                   slope, variant, _lib.stream_ptr(x.device))


def _conv_wino(lib, x, wp, bias, residual, out, strides, shape, slope, split, workspace=True, fallback=True):
    """3x3 / stride 1: F(2x2, 3x3) Winograd (csrc/sr_wino.hip; the fenced split-precision variant for `split` 1 / 2) on the
    weight `wp`, Winograd-packed in format `split`.  workspace=False: no split-K scratch is handed over, so the launcher never
    splits K (the training path); fallback=False: SR_ERR_UNSUPPORTED raises like any other error (no direct launch behind)."""
    isb, isp, osb, osp, rsb, rsp = strides
    b, ci, h, w, co = shape[:5]
    # 0 unless it splits K
    nbytes = _shape_query(lib, "sr_wino_splitk_workspace_bytes", b, h, w, ci, co, dev=x.device.index) if workspace else 0
    ws = _workspace(x.device, "wino_splitk", nbytes) if nbytes else None
    return _launch(x, shape, "sr_conv3x3_wino_nhwc_fwd", fallback and not split, lib.sr_conv3x3_wino_splitk_nhwc_fwd,
                   _lib.ptr(x), isb, isp, _lib.ptr(wp), _lib.ptr(bias), _lib.ptr(residual), rsb, rsp, _lib.ptr(out), osb, osp,
                   b, h, w, ci, co, slope, split, _lib.ptr(ws), nbytes, _lib.stream_ptr(x.device))


def _conv_direct(lib, x, wp, bias, residual, out, strides, shape, slope, pads, replicate, workspace=True):
    """Implicit-GEMM direct convolution (csrc/sr_conv.hip) on the packed weight `wp`: explicit zero `pads`, replicate or
    symmetric zero padding.  workspace=False: no split-K scratch, so the launcher never splits K (the training path)."""
    isb, isp, osb, osp, rsb, rsp = strides
    b, ci, h, w, co, k, s = shape[:7]
    args = (_lib.ptr(x), isb, isp, _lib.ptr(wp), _lib.ptr(bias), _lib.ptr(residual), rsb, rsp, _lib.ptr(out), osb, osp,
            b, h, w, ci, co, k, s)
    launch = lambda fn, *tail: _launch(x, shape, "sr_conv2d_nhwc_fwd", False, fn, *args, *tail, _lib.stream_ptr(x.device))
    if pads is not None:
        return launch(lib.sr_conv2d_padded_nhwc_fwd, *pads, slope)
    if replicate:
        return launch(lib.sr_conv2d_replicate_nhwc_fwd, slope)
    # 0 unless it may split K
    nbytes = _shape_query(lib, "sr_conv_splitk_workspace_bytes", b, h, w, ci, co, k, s, dev=x.device.index) if workspace else 0
    ws = _workspace(x.device, "conv_splitk", nbytes) if nbytes else None
    return launch(lib.sr_conv2d_splitk_nhwc_fwd, slope, _lib.ptr(ws), nbytes)


def basic_block(block, x, out=None):
    """BasicBlock.forward of the reference (modules/layers.py:68-85) as 2 (or 3) fused launches."""
    if not isinstance(block.bn1, nn.Identity) or not isinstance(block.bn2, nn.Identity):
        raise _lib.HipLibraryError("the HIP BasicBlock implements norm_layer=nn.Identity only (what SimpleRecon uses)")
    slope = block.relu.negative_slope
    x = as_nhwc(x, "BasicBlock input")
    t = conv2d(x, block.conv1, leaky=slope)
    identity = x if block.downsample is None else conv2d(x, block.downsample[0])
    return conv2d(t, block.conv2, residual=identity, leaky=slope, out=out)


def upsample2x(x, out=None):
    """Bilinear x2, align_corners=False (reference utils/generic_utils.py:96-105)."""
    x = as_nhwc(x, "upsample input")
    _lib.refuse_autograd(x)
    b, c, h, w = x.shape
    if out is None:
        out = empty_nhwc(b, c, 2 * h, 2 * w, x.device)
    elif tuple(out.shape) != (b, c, 2 * h, 2 * w) or not _is_nhwc_view(out):
        raise ValueError(f"`out` must be a channels-last view of shape {(b, c, 2 * h, 2 * w)}")
    if b == 0:
        return out
    isb, isp = _strides(x)
    osb, osp = _strides(out)
    _lib.call("sr_upsample2x_nhwc_fwd", x.device, x, isb, isp, out, osb, osp, b, h, w, c)
    return out


def exp(x):
    """Elementwise exp on a dense fp32 device tensor (any memory format; the result has the same strides)."""
    _lib.require_device_f32("exp input", x)
    if not (x.is_contiguous() or x.is_contiguous(memory_format=torch.channels_last)):
        x = x.contiguous()
    out = torch.empty_like(x)
    _lib.call("sr_exp_fwd", x.device, x, out, x.numel())
    return out


def copy_into(dst_view, src):
    """Copies a [B,C,H,W] tensor (any layout) into a channels-last slice (device-side strided copy)."""
    _lib.require_device_f32("copy source", src)
    dst_view.copy_(src)
    return dst_view


# ---------------------------------------------------------------- matching encoder ops --

_WORKSPACES = {}   # (device, tag) -> scratch tensor (grown on demand)


def _workspace(device, tag, nbytes):
    # one scratch buffer per (device, purpose, stream): launches on a stream are ordered, different streams must not share
    if _lib.capturing():
        # a HIP graph bakes the pointer in: give it memory from its own pool, never a cached buffer that a later eager
        # call may grow and drop
        return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
    key = (device, tag, _lib.stream_id(device))
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)
        _WORKSPACES[key] = ws
    return ws


def _pack_stem(conv, bn):
    """(packed weight, per-channel scale or None, shift or None) of the stem with `bn` and conv's bias folded into the
    epilogue."""
    wp = _pack("stem", conv.weight.detach().contiguous())
    scale = shift = None
    if bn is not None:
        scale, shift = bn_affine(bn)
    if conv.bias is not None:
        cb = conv.bias.detach()
        shift = (cb if scale is None else cb * scale) + (0 if shift is None else shift)
        shift = shift.contiguous()
    return wp, scale, shift


def stem7x7(image, conv: nn.Conv2d, bn=None, leaky=0.0, out=None):
    """act(bn(conv7x7_s2_p3(image))): encoder.conv1 + bn1 + relu of the ResNet stem (reference networks.py:176-179).
    image [B,3,H,W], any strides; returns channels-last [B,64,H/2,W/2] (or writes it into `out`, e.g. a batch slice
    of a larger buffer)."""
    _lib.require_device_f32("image", image)
    _lib.refuse_autograd(image, conv.weight)
    if conv.kernel_size != (7, 7) or conv.stride != (2, 2) or tuple(conv.padding) != (3, 3) or conv.groups != 1 \
            or conv.dilation != (1, 1) or conv.in_channels != 3 or conv.out_channels != 64 \
            or conv.padding_mode != "zeros":
        raise _lib.HipLibraryError(f"the HIP stem implements Conv2d(3, 64, 7, stride=2, padding=3) only, got {conv}")
    if image.dim() != 4 or image.shape[1] != 3:
        raise ValueError(f"stem expects [B,3,H,W], got {tuple(image.shape)}")
    _lib.require_device_f32("stem weight", conv.weight)
    wp, scale, shift = _cached(conv, "stem", _state_key(conv, bn), _pack_stem, conv, bn)
    b, _, h, w = image.shape
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    if out is None:
        out = empty_nhwc(b, 64, ho, wo, image.device)
    elif tuple(out.shape) != (b, 64, ho, wo) or not _is_nhwc_view(out):
        raise ValueError(f"`out` must be a channels-last view of shape {(b, 64, ho, wo)}")
    if b == 0:
        return out
    sb, sc, sy, sx = image.stride()
    osb, osp = _strides(out)
    rc = _timed(image.device, 2.0 * b * ho * wo * 64 * 147, (b, 3, h, w, 64, 7, 2), _lib.lib().sr_stem7x7_fwd, _lib.ptr(image),
                sb, sc, sy, sx, _lib.ptr(wp), _lib.ptr(scale), _lib.ptr(shift), -1.0 if leaky is None else float(leaky),
                _lib.ptr(out), osb, osp, b, h, w, 64, _lib.stream_ptr(image.device))
    _lib.check(rc, "sr_stem7x7_fwd")
    return out


def maxblurpool(x, out=None):
    """nn.MaxPool2d(2, stride=1) + antialiased_cnns.BlurPool(filt_size=4, stride=2), fused; channels-last (`out`: a
    channels-last view to write into, e.g. a channel slice of a larger buffer)."""
    x = as_nhwc(x, "maxblurpool input")
    b, c, h, w = x.shape
    if h < 4 or w < 4:
        raise ValueError(f"maxblurpool needs H, W >= 4, got {(h, w)}")
    ho, wo = (h - 2) // 2 + 1, (w - 2) // 2 + 1
    if out is None:
        out = empty_nhwc(b, c, ho, wo, x.device)
    elif tuple(out.shape) != (b, c, ho, wo) or not _is_nhwc_view(out):
        raise ValueError(f"`out` must be a channels-last view of shape {(b, c, ho, wo)}")
    if b == 0:
        return out
    isb, isp = _strides(x)
    osb, osp = _strides(out)
    _lib.call("sr_maxblurpool_nhwc_fwd", x.device, x, isb, isp, out, osb, osp, b, h, w, c)
    return out


def instance_norm(x, eps=1e-5, leaky=None, inplace=False):
    """nn.InstanceNorm2d (affine=False) [+ LeakyReLU(leaky)] on channels-last data."""
    x = as_nhwc(x, "instance_norm input")
    b, c, h, w = x.shape
    out = x if inplace else empty_nhwc(b, c, h, w, x.device)
    if b == 0 or h * w == 0:
        return out
    lib = _lib.lib()
    nbytes = lib.sr_instance_norm_workspace_bytes(b, h, w, c)
    ws = _workspace(x.device, "inorm", nbytes)
    isb, isp = _strides(x)
    osb, osp = _strides(out)
    _lib.call("sr_instance_norm_nhwc_fwd", x.device, x, isb, isp, out, osb, osp, b, h, w, c, eps,
              -1.0 if leaky is None else float(leaky), ws, ws.numel() * 4)
    return out


def instance_norm_stats(x, eps=1e-5):
    """Per-(image, channel) InstanceNorm statistics of a channels-last tensor: [B,2,C] = (mean, 1/sqrt(var + eps))."""
    x = as_nhwc(x, "instance_norm_stats input")
    b, c, h, w = x.shape
    stats = torch.empty((b, 2, c), dtype=torch.float32, device=x.device)
    if b == 0:
        return stats
    lib = _lib.lib()
    ws = _workspace(x.device, "inorm", lib.sr_instance_norm_workspace_bytes(b, h, w, c))
    isb, isp = _strides(x)
    _lib.call("sr_instance_norm_stats_nhwc", x.device, x, isb, isp, b, h, w, c, eps, stats, ws, ws.numel() * 4)
    return stats


def conv1x1_stats(x, conv: nn.Conv2d, eps=1e-5):
    """(conv(x), InstanceNorm statistics [B,2,C] of conv(x)) for the matching encoder's Conv2d(64, 128, 1) ->
    InstanceNorm2d pair (reference networks.py:187-188): the statistics come out of the convolution's own pass."""
    _lib.refuse_autograd(x, conv.weight)
    x = as_nhwc(x, "conv input")
    b, ci, h, w = x.shape
    co = conv.out_channels
    if conv.kernel_size != (1, 1) or conv.stride != (1, 1) or tuple(conv.padding) != (0, 0) or conv.groups != 1 \
            or (ci, co) != (64, 128) or ci != conv.in_channels:
        raise _lib.HipLibraryError(f"conv1x1_stats needs Conv2d(64, 128, 1), got {conv} for {ci} channels")
    out = empty_nhwc(b, co, h, w, x.device)
    stats = torch.empty((b, 2, co), dtype=torch.float32, device=x.device)
    if b == 0:
        return out, stats
    lib = _lib.lib()
    ws = _workspace(x.device, "c1s", lib.sr_conv1x1_stats_workspace_bytes(b, h, w, co))
    weight = conv.weight.detach().reshape(co, ci).contiguous()   # [128][64] rows, whatever the module's memory format
    bias = conv.bias.detach() if conv.bias is not None else None
    isb, isp = _strides(x)
    osb, osp = _strides(out)
    rc = _timed(x.device, 2.0 * b * h * w * co * ci, (b, ci, h, w, co, 1, 1), lib.sr_conv1x1_stats_nhwc_fwd, _lib.ptr(x), isb,
                isp, _lib.ptr(weight), _lib.ptr(bias), _lib.ptr(out), osb, osp, b, h, w, ci, co, eps, _lib.ptr(stats),
                _lib.ptr(ws), ws.numel() * 4, _lib.stream_ptr(x.device))
    _lib.check(rc, "sr_conv1x1_stats_nhwc_fwd")
    return out, stats


def _pack_c16(conv):
    return _pack("conv3x3_c16", conv.weight.detach().contiguous()), (conv.bias.detach() if conv.bias is not None else None)


def conv3x3_c16(x, conv: nn.Conv2d, in_stats=None, in_leaky=None, leaky=None):
    """conv3x3 (<= 16 output channels, zero or replicate padding) of act(InstanceNorm(x)) where the normalisation
    (statistics `in_stats` from instance_norm_stats) and its LeakyReLU are applied while the input is staged."""
    _lib.refuse_autograd(x, conv.weight)
    x = as_nhwc(x, "conv input")
    b, ci, h, w = x.shape
    co = conv.out_channels
    if conv.kernel_size != (3, 3) or conv.stride != (1, 1) or tuple(conv.padding) != (1, 1) or conv.groups != 1 \
            or conv.dilation != (1, 1) or conv.padding_mode not in ("zeros", "replicate") or co > 16 or ci % 32 \
            or ci != conv.in_channels:
        raise _lib.HipLibraryError(f"conv3x3_c16 needs Conv2d(32k, <=16, 3, padding=1), got {conv} for {ci} channels")
    wp, bias = _cached(conv, "c16", _state_key(conv, None), _pack_c16, conv)
    if in_stats is not None and (tuple(in_stats.shape) != (b, 2, ci) or not in_stats.is_contiguous()):
        raise ValueError(f"in_stats must be a contiguous [{b}, 2, {ci}] tensor")
    out = empty_nhwc(b, co, h, w, x.device)
    if b == 0:
        return out
    isb, isp = _strides(x)
    osb, osp = _strides(out)
    rc = _timed(x.device, 2.0 * b * h * w * co * ci * 9, (b, ci, h, w, co, 3, 1), _lib.lib().sr_conv3x3_c16_nhwc_fwd,
                _lib.ptr(x), isb, isp, _lib.ptr(in_stats), -1.0 if in_leaky is None else float(in_leaky), _lib.ptr(wp),
                _lib.ptr(bias), _lib.ptr(out), osb, osp, b, h, w, ci, co, int(conv.padding_mode == "replicate"),
                -1.0 if leaky is None else float(leaky), _lib.stream_ptr(x.device))
    _lib.check(rc, "sr_conv3x3_c16_nhwc_fwd")
    return out


# ---- MBConv pieces of the image-prior encoder (csrc/sr_mbconv.hip) -----------------------------------------------

def _pack_dw(conv, bn):
    w, bias = _effective_weight(conv, bn)                      # [C, 1, 3, 3]
    return w.reshape(conv.in_channels, 9).t().contiguous(), (bias.contiguous() if bias is not None else None)


def packed_dw_weight(conv: nn.Conv2d, bn=None):
    """([9, C] tap-major depthwise weight with the eval-mode BatchNorm scale folded in, bias); cached."""
    _lib.require_device_f32("depthwise conv weight", conv.weight)
    c = conv.in_channels
    if conv.kernel_size != (3, 3) or conv.groups != c or conv.out_channels != c or conv.dilation != (1, 1) \
            or conv.padding_mode != "zeros":
        raise _lib.HipLibraryError(f"unsupported depthwise Conv2d configuration for the HIP path: {conv}")
    return _cached(conv, "dw", _state_key(conv, bn), _pack_dw, conv, bn)


def dwconv3x3(x, conv: nn.Conv2d, bn=None, leaky=None, act=None, tf_same=False, want_pool=False, pads=None):
    """act(bn(depthwise_conv3x3(x))) on a channels-last view; with want_pool also returns the per-band partial sums
    of the result ([B, bands, C]) from which `se_gate` finishes the squeeze-excite average pool."""
    _lib.refuse_autograd(x, conv.weight)
    x = as_nhwc(x, "depthwise conv input")
    b, c, h, w = x.shape
    if c != conv.in_channels:
        raise ValueError(f"depthwise conv expects {conv.in_channels} channels, got {c}")
    s = conv.stride[0]
    if conv.stride[0] != conv.stride[1] or s not in (1, 2):
        raise _lib.HipLibraryError(f"unsupported stride {conv.stride}")
    if pads is None and not tf_same and tuple(conv.padding) != (1, 1):
        raise _lib.HipLibraryError(f"unsupported padding {conv.padding}")
    if pads is None:
        pads = tf_same_pads(h, w, 3, s) if tf_same else (1, 1, 1, 1)
    ho, wo = (h + pads[0] + pads[2] - 3) // s + 1, (w + pads[1] + pads[3] - 3) // s + 1
    w9c, bias = packed_dw_weight(conv, bn)
    lib = _lib.lib()
    out = empty_nhwc(b, c, ho, wo, x.device)
    bands = lib.sr_dwconv3x3_pool_bands(ho)
    pool = torch.empty((b, bands, c), dtype=torch.float32, device=x.device) if want_pool else None
    if b > 0:
        isb, isp = _strides(x)
        osb, osp = _strides(out)
        _lib.call("sr_dwconv3x3_nhwc_fwd", x.device, x, isb, isp, w9c, bias, out, osb, osp, pool, b, h, w, c, s, *pads,
                  _act_code(leaky, act))
    return (out, pool) if want_pool else out


def se_gate(pool_partial, pixels, conv_reduce: nn.Conv2d, conv_expand: nn.Conv2d):
    """sigmoid(conv_expand(silu(conv_reduce(mean)))) per image from dwconv3x3's partial sums: [B, C] gates."""
    _lib.require_device_f32("pool partial sums", pool_partial)
    b, bands, c = pool_partial.shape
    rd = conv_reduce.out_channels
    if conv_reduce.kernel_size != (1, 1) or conv_expand.kernel_size != (1, 1) or conv_reduce.in_channels != c \
            or conv_expand.in_channels != rd or conv_expand.out_channels != c:
        raise _lib.HipLibraryError("squeeze-excite expects 1x1 convs C -> rd -> C")
    _lib.refuse_autograd(pool_partial, conv_reduce.weight, conv_expand.weight)
    gate = torch.empty((b, c), dtype=torch.float32, device=pool_partial.device)
    if b == 0:
        return gate
    w1 = conv_reduce.weight.detach().reshape(rd, c)
    w2 = conv_expand.weight.detach().reshape(c, rd)
    b1 = conv_reduce.bias.detach() if conv_reduce.bias is not None else None
    b2 = conv_expand.bias.detach() if conv_expand.bias is not None else None
    for t in (w1, w2):
        _lib.require_device_f32("squeeze-excite weight", t)
    _lib.call("sr_se_gate_fwd", gate.device, pool_partial.contiguous(), bands, pixels, w1.contiguous(), b1, w2.contiguous(),
              b2, gate, b, c, rd)
    return gate


def _pack_rgb(conv, bn):
    """([27, Cout] weight with `bn` folded in, bias)."""
    wt, bias = _effective_weight(conv, bn)                                     # [Cout, 3, 3, 3]
    w27 = wt.permute(2, 3, 1, 0).reshape(27, conv.out_channels).contiguous()   # [ky][kx][ci][Cout]
    return w27, (bias.contiguous() if bias is not None else None)


def rgb_stem3x3s2(image, conv: nn.Conv2d, bn=None, act=None, leaky=None, tf_same=True):
    """act(bn(conv3x3_s2(image))) for a 3-channel image (EfficientNetV2's conv_stem): a VALU kernel that reads the image
    through its strides; returns a channels-last [B, Cout, Ho, Wo] tensor.  Falls back to conv2d for other layers."""
    _lib.require_device_f32("image", image)
    _lib.refuse_autograd(image, conv.weight)
    if conv.kernel_size != (3, 3) or conv.stride != (2, 2) or conv.in_channels != 3 or conv.groups != 1 or \
            conv.out_channels != 24 or image.dim() != 4 or image.shape[1] != 3:
        return conv2d(image, conv, bn=bn, act=act, leaky=leaky, tf_same=tf_same)
    b, _, h, w = image.shape
    pads = tf_same_pads(h, w, 3, 2) if tf_same else (1, 1, 1, 1)
    ho, wo = (h + pads[0] + pads[2] - 3) // 2 + 1, (w + pads[1] + pads[3] - 3) // 2 + 1
    w27, bias = _cached(conv, "rgb", _state_key(conv, bn), _pack_rgb, conv, bn)
    out =empty_nhwc(b, conv.out_channels, ho, wo, image.device)
    if b == 0:
        return out
    sb, sc, sy, sx = image.stride()
    osb, osp = _strides(out)
    _lib.call("sr_rgb_stem3x3s2_fwd", image.device, image, sb, sc, sy, sx, w27, bias, out, osb, osp, b, h, w,
              conv.out_channels, pads[0], pads[1], ho, wo, _act_code(leaky, act))
    return out


def se_gates(pool_partial, pixels, conv_reduce: nn.Conv2d, conv_expand: nn.Conv2d):
    """[B, C] squeeze-excite gates from dwconv3x3's partial sums (two short launches); the consumer -- conv2d(..., gate=) --
    applies them to its input while loading it, so the gated map is never written."""
    _lib.require_device_f32("pool partial sums", pool_partial)
    b, bands, c = pool_partial.shape
    rd = conv_reduce.out_channels
    if conv_reduce.kernel_size != (1, 1) or conv_expand.kernel_size != (1, 1) or conv_reduce.in_channels != c \
            or conv_expand.in_channels != rd or conv_expand.out_channels != c or not pool_partial.is_contiguous():
        raise _lib.HipLibraryError("squeeze-excite expects 1x1 convs C -> rd -> C and contiguous [B, bands, C] partial sums")
    _lib.refuse_autograd(pool_partial, conv_reduce.weight, conv_expand.weight)
    gate = torch.empty((b, c), dtype=torch.float32, device=pool_partial.device)
    if b == 0:
        return gate
    hidden = torch.empty((b, rd), dtype=torch.float32, device=pool_partial.device)
    w1, w2 = conv_reduce.weight.detach(), conv_expand.weight.detach()
    if not (w1.is_contiguous() and w2.is_contiguous()):
        w1, w2 = w1.contiguous(), w2.contiguous()
    b1 = conv_reduce.bias.detach() if conv_reduce.bias is not None else None
    b2 = conv_expand.bias.detach() if conv_expand.bias is not None else None
    _lib.call("sr_se_gate2_fwd", gate.device, pool_partial, bands, pixels, w1, b1, w2, b2, hidden, gate, b, c, rd)
    return gate


def se_scale_(x, pool_partial, conv_reduce: nn.Conv2d, conv_expand: nn.Conv2d, want_gate=False):
    """x *= squeeze-excite gate, in place on a channels-last view (se_gate + scale_channels_ in two short launches)."""
    _lib.require_device_f32("pool partial sums", pool_partial)
    if not _is_nhwc_view(x):
        raise ValueError("se_scale_ needs a channels-last view")
    b, c, h, w = x.shape
    rd = conv_reduce.out_channels
    if conv_reduce.kernel_size != (1, 1) or conv_expand.kernel_size != (1, 1) or conv_reduce.in_channels != c \
            or conv_expand.in_channels != rd or conv_expand.out_channels != c or pool_partial.shape[0] != b \
            or pool_partial.shape[2] != c or not pool_partial.is_contiguous():
        raise _lib.HipLibraryError("squeeze-excite expects 1x1 convs C -> rd -> C and [B, bands, C] partial sums")
    _lib.refuse_autograd(x, pool_partial, conv_reduce.weight, conv_expand.weight)
    gate = torch.empty((b, c), dtype=torch.float32, device=x.device) if want_gate else None
    if b == 0:
        return (x, gate) if want_gate else x
    hidden = torch.empty((b, rd), dtype=torch.float32, device=x.device)
    w1, w2 = conv_reduce.weight.detach(), conv_expand.weight.detach()
    if not (w1.is_contiguous() and w2.is_contiguous()):
        w1, w2 = w1.contiguous(), w2.contiguous()
    b1 = conv_reduce.bias.detach() if conv_reduce.bias is not None else None
    b2 = conv_expand.bias.detach() if conv_expand.bias is not None else None
    sb, sp = _strides(x)
    _lib.call("sr_se_scale_nhwc_fwd", x.device, pool_partial, pool_partial.shape[1], w1, b1, w2, b2, hidden, x, sb, sp, x, sb,
              sp, gate, b, h, w, c, rd)
    return (x, gate) if want_gate else x


def scale_channels_(x, gate):
    """x[b, c, :, :] *= gate[b, c] in place on a channels-last view."""
    _lib.require_device_f32("gate", gate)
    if not _is_nhwc_view(x):
        raise ValueError("scale_channels_ needs a channels-last view")
    _lib.refuse_autograd(x, gate)
    b, c, h, w = x.shape
    if tuple(gate.shape) != (b, c) or not gate.is_contiguous():
        raise ValueError(f"gate must be a contiguous [{b}, {c}] tensor")
    if b == 0:
        return x
    sb, sp = _strides(x)
    _lib.call("sr_scale_channels_nhwc_fwd", x.device, x, sb, sp, gate, x, sb, sp, b, h, w, c)
    return x


def add_(y, x):
    """y += x on channels-last views (same shape)."""
    _lib.require_device_f32("y", y)
    x = as_nhwc(x, "x")
    if not _is_nhwc_view(y) or tuple(x.shape) != tuple(y.shape):
        raise ValueError("add_ needs two channels-last views of the same shape")
    _lib.refuse_autograd(x, y)
    b, c, h, w = y.shape
    if b == 0:
        return y
    ysb, ysp = _strides(y)
    xsb, xsp = _strides(x)
    _lib.call("sr_add_nhwc_fwd", y.device, y, ysb, ysp, x, xsb, xsp, y, ysb, ysp, b, h, w, c)
    return y
