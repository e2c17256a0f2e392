"""Differentiable conv-stack operators: the training path of BasicBlock / CVEncoder / DepthDecoderPP (reference
train.py:126-145 runs autograd through modules/layers.py:24-85 and modules/networks.py:20-127), and the convolution layer
(`_ConvBiasAct`) the two encoders train through as well (train_ops.conv; their normalisation, pooling, depthwise and
squeeze-excite operators are in train_ops).

torch.autograd is the tape (plumbing); every arithmetic step, forward and backward, is a HIP kernel:
  forward        the same MFMA kernels as inference (direct / Winograd), weights packed per call (they change every step);
  data gradient  the forward kernels on the flipped, transposed weight (stride 2: on the zero-stuffed output gradient);
  weight / bias  csrc/sr_conv_bwd.hip (MFMA split over pixels, partial slabs + ordered reduce: deterministic);
  LeakyReLU      from the saved output; bilinear x2: its adjoint kernel.
Under torch.autocast the layer stays on fp32 kernels unless the switches below put 16-bit storage, 16-bit kernel I/O
(sr_conv3x3_wino_io_nhwc_fwd, sr_pw_conv_io_nhwc_fwd) or the 16-bit MFMA kernels (csrc/sr_conv16.hip, csrc/sr_conv16_wgrad.hip)
on its path.  Gradients are pinned to the reference's own autograd (tests/golden/grad_block_*.npz, grad_cv_encoder_narrow.npz,
grad_decoder_narrow.npz); which kernels the layer launches, for every setting of the switches, to
tests/golden/conv_layer_trace.json.gz."""
import functools
import os

import torch
from torch import nn

from . import _lib
from .ops import _act_code, _conv_direct, _conv_wino, _is_nhwc_view, _pack, _strides, _workspace, as_nhwc, empty_nhwc


# torch.autocast compatibility (the reference trains under 16-bit autocast, options.py:100-101, train.py:132).  Every
# differentiable operator runs with autocast off inside and records on ctx whether its caller was inside an autocast region.
# `_amp_fwd` / `_amp_bwd` (every operator but the conv layer) cast floating-point CUDA inputs that arrive in fp16 / bf16 to
# fp32 at the operator's entry (a differentiable cast: gradients go back in the caller's dtype): fp32 kernels whatever the
# autocast state.  `_amp_state_fwd` / `_amp_state_bwd` (`_ConvBiasAct`) leave the inputs alone: the layer decides what its
# kernels read and write.
_amp_cast_fwd = torch.amp.custom_fwd(device_type="cuda", cast_inputs=torch.float32)
_amp_bwd = torch.amp.custom_bwd(device_type="cuda")


def _autocast_off(fn):
    @functools.wraps(fn)
    def wrapper(ctx, *args, **kwargs):
        with torch.autocast(device_type="cuda", enabled=False):
            return fn(ctx, *args, **kwargs)
    return wrapper


def _recording_autocast(body):
    """`body` (a forward with autocast already dealt with) behind a note on ctx of the caller's autocast state and dtype: what
    `_stash` and `_ConvBiasAct` go by."""
    @functools.wraps(body)
    def wrapper(ctx, *args, **kwargs):
        on = torch.is_autocast_enabled("cuda")
        ctx._sr_autocast = on
        ctx._sr_autocast_dtype = torch.get_autocast_dtype("cuda") if on else None
        return body(ctx, *args, **kwargs)
    return wrapper


def _amp_fwd(fwd):
    return _recording_autocast(_amp_cast_fwd(fwd))


def _amp_state_fwd(fwd):
    return _recording_autocast(_autocast_off(fwd))


_amp_state_bwd = _autocast_off


# The four 16-bit switches of the layer under torch.autocast.  All are read at call time (tests, scripts and
# experimental.autocast_mfma16 set the module attributes) and all default to off: an autocast step then runs the fp32 step's
# kernels.
#
# STORE_HALF (SR_AUTOCAST_HALF_STORAGE): what autograd SAVES for the backward pass -- the bulk of a training step's memory -- is
# stored in the autocast dtype and widened again when a backward kernel needs fp32 (`_stash` / `_unstash`, shared with
# train_ops).  A tensor saved by several operators (a producer saves its output for the activation's derivative, the consumer
# saves it as its input) is narrowed once and shared.  Tensors below 4096 elements and parameters are left alone.
STORE_HALF = os.environ.get("SR_AUTOCAST_HALF_STORAGE", "0") != "0"
# HALF_IO (SR_AUTOCAST_HALF_IO): inside an autocast region `_ConvBiasAct` reads and writes its activations in the autocast
# dtype, like the reference's `precision: 16` training (options.py:100-101, train.py:132).  The Winograd and pointwise kernels
# load four 16-bit channels as one 8-byte access, widen them, accumulate in fp32 (fp32 weights, fp32 MFMA) and round once on
# the way out; stride-2 and explicitly padded convolutions convert at the boundary of the fp32 kernel.  The backward kernels
# run on fp32 copies of the saved tensors.
# Why both are opt-in: together they bring the peak from 5.9 to 3.8 GiB (batch 2, 640x480, 7 views) and cost time, because
# every saved tensor is narrowed once and widened once by cast kernels (892 + 593 launches per step).  Training step
# (scripts/train_step_micro.py 2, profiles/r06_train_autocast.txt): fp32 77.7 ms; bf16 autocast with storage + I/O 87.0,
# storage only 85.8, I/O only 83.1, neither 78.4.
HALF_IO = os.environ.get("SR_AUTOCAST_HALF_IO", "0") != "0"
_IO_CODE = {torch.float16: 1, torch.bfloat16: 2}
# MFMA16 (SR_AUTOCAST_MFMA16): where HALF_IO has put 16-bit activations on the path, 3x3 convolutions at stride 1 and 2 and 1x1
# convolutions multiply on the 16-bit matrix pipe (csrc/sr_conv16.hip: weights rounded once to the activation dtype, fp32
# accumulation, bias / residual / LeakyReLU in fp32, one rounding on the way out).  A layer whose forward ran there takes its
# data gradient there as well, on the post-activation gradient cast to the layer's dtype.  1 = the layers sr_conv16_supported
# AND sr_conv16_prefers accept (the measured rule, profiles/r07_conv16.txt), 2 = every supported layer (tests, A/B runs).
# fp16 (not bf16) needs a loss scaler: the 16-bit data gradient underflows otherwise.
MFMA16 = int(os.environ.get("SR_AUTOCAST_MFMA16", "0") or 0)
# MFMA16_WGRAD (SR_AUTOCAST_MFMA16_WGRAD): the backward of a layer whose forward ran on the 16-bit MFMA kernel makes no fp32
# copy of the saved input and output.  sr_act_bwd_bias16_nhwc reads the arriving gradient (fp32 or 16-bit) and the saved
# output and writes the 16-bit post-activation gradient and the fp32 bias gradient; sr_conv16_wgrad_nhwc multiplies the saved
# input with it on the 16-bit matrix pipe (csrc/sr_conv16_wgrad.hip: exact products, fp32 accumulation, deterministic); the
# data gradient consumes the same 16-bit gradient (stride 2: around the fp32 zero-stuffing kernel).  1 = the layers
# sr_conv16_wgrad_supported AND sr_conv16_wgrad_prefers accept (the measured rule, profiles/r08_conv16_wgrad.txt), 2 = every
# supported layer.
MFMA16_WGRAD = int(os.environ.get("SR_AUTOCAST_MFMA16_WGRAD", "0") or 0)
# FUSED_ACT_BIAS (SR_FUSED_ACT_BIAS, default on): LeakyReLU' and the bias gradient of the fp32 backward in one float4 pass
# (sr_act_bwd_bias_nhwc); 0, or Cout % 4 != 0: separate sr_act_bwd and sr_bias_grad_nhwc launches.
FUSED_ACT_BIAS = os.environ.get("SR_FUSED_ACT_BIAS", "1") != "0"


def _nhwc_any(t, name):
    """A channels-last view of a CUDA tensor of any of the I/O dtypes (fp32 / fp16 / bf16)."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        raise _lib.HipLibraryError(f"{name}: expected a CUDA fp32 / fp16 / bf16 tensor, got {getattr(t, 'dtype', type(t))} on "
                                   f"{getattr(t, 'device', '?')}")
    if t.dim() != 4:
        raise ValueError(f"{name} must be [B,C,H,W], got {tuple(t.shape)}")
    return t if _is_nhwc_view(t) else t.contiguous(memory_format=torch.channels_last)


def _stash(ctx, *tensors):
    half = STORE_HALF and getattr(ctx, "_sr_autocast", False)
    dt = getattr(ctx, "_sr_autocast_dtype", None)
    keep, flags = [], []
    for t in tensors:
        narrow = half and isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 4 and \
            not isinstance(t, nn.Parameter) and t.numel() >= 4096
        if narrow:
            # the 16-bit copy is shared between the operators that save this tensor; it is valid only for the very
            # contents it was made from (an input refreshed in place with copy_ must be narrowed again)
            rec = getattr(t, "_sr_narrow", None)
            if rec is None or rec[0] != t._version or rec[1] != t.data_ptr() or rec[2].dtype != dt:
                rec = (t._version, t.data_ptr(), t.detach().to(dt))
                t._sr_narrow = rec
            keep.append(rec[2])
        else:
            keep.append(t)
        flags.append(narrow)
    ctx.save_for_backward(*keep)
    ctx._sr_stash_flags = flags


def _unstash(ctx):
    return tuple(t.float() if (f and t is not None) else t for t, f in zip(ctx.saved_tensors, ctx._sr_stash_flags))


def grad_wanted(*tensors_or_modules):
    """True when autograd is recording and any tensor / module parameter asks for a gradient."""
    if not torch.is_grad_enabled():
        return False
    for t in tensors_or_modules:
        if isinstance(t, torch.Tensor):
            if t.requires_grad:
                return True
        elif isinstance(t, nn.Module):
            if any(p.requires_grad for p in t.parameters()):
                return True
        elif isinstance(t, (list, tuple)):
            if grad_wanted(*t):
                return True
    return False


# Every registration of a submodule anywhere in the process (add_module / attribute assignment: SyncBatchNorm conversion,
# BatchNorm fusion, a swapped block) bumps this counter through torch's global registration hook; cached layer lists carry the
# value they were gathered under.
_TREE_EPOCH = [0]


def _bump_tree_epoch(module, name, submodule):
    _TREE_EPOCH[0] += 1


torch.nn.modules.module.register_module_module_registration_hook(_bump_tree_epoch)


def any_batchnorm_training(module):
    """True if a batch-norm layer of `module` (BatchNorm2d, SyncBatchNorm, ... -- any `_BatchNorm`) is in training mode (batch
    statistics cannot be folded into the conv weights).  The layer list is gathered once per module TREE: walking `modules()`
    costs ~1 ms per forward on the EfficientNetV2-S pyramid, so the list is cached together with the process-wide submodule
    registration count it was gathered under -- replacing a layer anywhere (also deep in the tree, which r04's key of
    (training, number of direct children) missed) invalidates it, and every cached layer is re-checked against its parent's
    `_modules` entry (mutations the hook cannot see).  The layers' own `training` flags are read on every call."""
    rec = module.__dict__.get("_sr_bn_layers")
    if rec is not None and rec[0] == _TREE_EPOCH[0]:
        # the registration hook does not see direct mutations of `_modules` (del m.bn, ModuleList.__delitem__ / insert, fx or
        # quantisation swaps): every cached layer must still sit where it was found (~100 dict lookups)
        for parent, name, layer in rec[1]:
            if parent._modules.get(name) is not layer:
                rec = None
                break
    if rec is None or rec[0] != _TREE_EPOCH[0]:
        found = []
        for parent in module.modules():
            for name, child in parent._modules.items():
                if isinstance(child, nn.modules.batchnorm._BatchNorm):
                    found.append((parent, name, child))
        if isinstance(module, nn.modules.batchnorm._BatchNorm):
            found.append((_Holder(module), "self", module))
        rec = (_TREE_EPOCH[0], found)
        module.__dict__["_sr_bn_layers"] = rec
    for _, _, m in rec[1]:
        if m.training:
            return True
    return False


class _Holder:
    """Stand-in parent for a batch-norm layer that is itself the root of the query."""
    def __init__(self, m):
        self._modules = {"self": m}


def _dense_nhwc(t, any_dtype=False):
    """Channels-last, dense (pixel stride = C): what the elementwise backward kernels and the wgrad staging expect.  fp32, or
    (any_dtype) any of the I/O dtypes."""
    t = _nhwc_any(t, "gradient") if any_dtype else as_nhwc(t, "gradient")
    c, h, w = t.shape[1], t.shape[2], t.shape[3]
    if t.stride(1) != 1 or t.stride(3) != c or t.stride(2) != w * c or (t.shape[0] > 1 and t.stride(0) != h * w * c):
        t = t.contiguous(memory_format=torch.channels_last)
        if t.shape[0] > 1 and t.stride(0) != h * w * c:   # (contiguous() keeps a batch-strided view whose images are dense)
            t = t.clone(memory_format=torch.channels_last)
    return t


def _rows_aligned(t, nbytes):
    """None, or a channels-last view whose pixel rows all start `nbytes`-aligned (nbytes / element size channels per access)."""
    return t is None or (t.data_ptr() % nbytes == 0 and all(st % (nbytes // t.element_size()) == 0 for st in _strides(t)))


def _mfma16_selects(b, h, w, ci, co, k, stride, pads):
    """The routing predicate of MFMA16 on a layer's shape: never with the switch at 0, never for explicit `pads`."""
    mode = MFMA16
    if not mode or pads is not None or b <= 0:
        return False
    lib = _lib.lib()
    if not lib.sr_conv16_supported(b, h, w, ci, co, k, stride):
        return False
    return mode >= 2 or bool(lib.sr_conv16_prefers(b, h, w, ci, co, k, stride))


def _wgrad16_selects(b, h, w, ci, co, k, stride, pads):
    """The routing predicate of MFMA16_WGRAD on a layer's shape: never with the switch at 0, never for explicit `pads`."""
    mode = MFMA16_WGRAD
    if not mode or pads is not None or b <= 0:
        return False
    lib = _lib.lib()
    if not lib.sr_conv16_wgrad_supported(b, h, w, ci, co, k, stride):
        return False
    return mode >= 2 or bool(lib.sr_conv16_wgrad_prefers(b, h, w, ci, co, k, stride))


def _conv16_routes(x, weight, stride, residual, pads):
    """True when _conv_raw_io takes this call (16-bit channels-last views `x`, `residual`) to the 16-bit MFMA kernel."""
    b, ci, h, w = x.shape
    co, _, k, _ = weight.shape
    return x.dtype in _IO_CODE and _mfma16_selects(b, h, w, ci, co, k, stride, pads) and _rows_aligned(x, 16) and \
        (residual is None or (residual.dtype == x.dtype and _rows_aligned(residual, 16)))


def _conv16(x, weight, bias, stride, residual, slope, out_f32=False):
    """act(conv(x, weight) + bias [+ residual]) on sr_conv16_nhwc_fwd: `x` / `residual` fp16 or bf16 channels-last views, the
    fp32 weight tensor rounded to that dtype and packed on the fly, output in the same dtype or (out_f32) fp32."""
    dt = x.dtype
    b, ci, h, w = x.shape
    co, _, k, _ = weight.shape
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    out = torch.empty((b, co, ho, wo), dtype=torch.float32 if out_f32 else dt, device=x.device,
                      memory_format=torch.channels_last)
    wp = torch.empty(_lib.lib().sr_conv16_packed_weight_bytes(co, ci, k), dtype=torch.uint8, device=x.device)
    _lib.call("sr_conv16_pack_weights", x.device, weight.detach().float().contiguous(), co, ci, k, _IO_CODE[dt], wp)
    bd = bias.detach().float().contiguous() if bias is not None else None
    rsb, rsp = _strides(residual) if residual is not None else (0, 0)
    _lib.call("sr_conv16_nhwc_fwd", x.device, x, *_strides(x), wp, bd, residual, rsb, rsp, out, *_strides(out), b, h, w, ci, co,
              k, stride, _act_code(slope, None), _IO_CODE[dt], 0 if out_f32 else _IO_CODE[dt])
    return out


def _conv_raw_io(x, weight, bias, stride, residual, slope, pads, mfma16=None):
    """_conv_raw on fp16 / bf16 activations: the 16-bit MFMA kernel where MFMA16 selects the layer (3x3 at stride 1 and 2, 1x1;
    `mfma16`: that decision, for a caller that has made it on these channels-last views already); else 16-bit kernel I/O where
    the kernel has it (3x3 / stride 1 through Winograd, 1x1 / stride 1 through the pointwise GEMM), boundary conversion around
    the fp32 kernel otherwise."""
    dt = x.dtype
    x = _nhwc_any(x, "conv input")
    b, ci, h, w = x.shape
    co, ci_w, k, _ = weight.shape
    if ci_w != ci:
        raise ValueError(f"conv weight expects {ci_w} input channels, got {ci}")
    if residual is not None:
        residual = _nhwc_any(residual if residual.dtype == dt else residual.to(dt), "residual")
    if _conv16_routes(x, weight, stride, residual, pads) if mfma16 is None else mfma16:
        return _conv16(x, weight, bias, stride, residual, slope)
    wino = pads is None and stride == 1 and k == 3 and b > 0 and ci % 4 == 0 and co % 4 == 0 and \
        bool(_lib.lib().sr_conv_prefers_wino(b, h, w, ci, co, k, stride))
    pw = pads is None and stride == 1 and k == 1 and b > 0 and ci % 4 == 0
    if not ((wino or pw) and _rows_aligned(x, 8) and _rows_aligned(residual, 8)):
        y = _conv_raw(x.float(), weight, bias, stride, residual.float() if residual is not None else None, slope, pads)
        return y.to(dt)
    if wino and _lib.get_option("SR_WINO_SPLIT") != 0:
        raise _lib.HipLibraryError("the split-precision Winograd variant (SR_WINO_SPLIT) takes fp32 tensors: no 16-bit I/O")
    out = torch.empty((b, co, h, w), dtype=dt, device=x.device, memory_format=torch.channels_last)
    wp = _pack("wino", weight.detach().float().contiguous(), 0) if wino else _pack("conv", weight.detach().float().contiguous())
    bd = bias.detach().float().contiguous() if bias is not None else None
    rsb, rsp = _strides(residual) if residual is not None else (0, 0)
    head = (x, *_strides(x), wp, bd, residual, rsb, rsp, out, *_strides(out), b)
    if wino:
        _lib.call("sr_conv3x3_wino_io_nhwc_fwd", x.device, *head, h, w, ci, co, _act_code(slope, None), _IO_CODE[dt])
    else:
        _lib.call("sr_pw_conv_io_nhwc_fwd", x.device, *head, h * w, ci, co, _act_code(slope, None), _IO_CODE[dt])
    return out


def _conv_raw(x, weight, bias, stride, residual=None, slope=None, pads=None):
    """act(conv(x, weight) + bias [+ residual]) on the inference launchers of ops with a weight TENSOR [Co, Ci, k, k]
    (packed on the fly; padding k // 2, or explicit (top, left, bottom, right) zero `pads`).  Winograd F(2x2) where the
    library prefers it, else the direct kernel; never F(4x4), the pointwise GEMM or split-K."""
    if x.dtype in _IO_CODE:
        return _conv_raw_io(x, weight, bias, stride, residual, slope, pads)
    lib = _lib.lib()
    x = as_nhwc(x, "conv input")
    b, ci, h, w = x.shape
    co, ci_w, k, _ = weight.shape
    if ci_w != ci:
        raise ValueError(f"conv weight expects {ci_w} input channels, got {ci}")
    pt, pl, pb, pr = pads if pads is not None else (k // 2,) * 4
    ho, wo = (h + pt + pb - k) // stride + 1, (w + pl + pr - k) // stride + 1
    out = empty_nhwc(b, co, ho, wo, x.device)
    if b == 0:
        return out
    use_wino = pads is None and stride == 1 and k == 3 and bool(lib.sr_conv_prefers_wino(b, h, w, ci, co, k, stride))
    split = _lib.get_option("SR_WINO_SPLIT") if use_wino else 0   # read once: the pack and the launch take this value
    wp = _pack("wino", weight.detach().contiguous(), split) if use_wino else _pack("conv", weight.detach().contiguous())
    if residual is not None:
        residual = as_nhwc(residual, "residual")
    bd = bias.detach().contiguous() if bias is not None else None
    strides = (*_strides(x), *_strides(out), *(_strides(residual) if residual is not None else (0, 0)))
    # (the shape also goes into ops.PROFILE with the kernel the launch ran: the data gradient's launches are told apart by it)
    shape = (b, ci, h, w, co, k, stride, ho, wo, residual is not None)
    if use_wino:
        _conv_wino(lib, x, wp, bd, residual, out, strides, shape, _act_code(slope, None), split, workspace=False, fallback=False)
    else:
        _conv_direct(lib, x, wp, bd, residual, out, strides, shape, _act_code(slope, None), pads, False, workspace=False)
    return out


def _grad16(ctx, g, x, weight, out):
    """The predicate of the backward on 16-bit operands (MFMA16_WGRAD): the arriving gradient (fp32 or the layer's dtype) as a dense
    channels-last tensor when the layer's forward ran on sr_conv16_nhwc_fwd, what it saved is 16-bit, the switch selects its shape
    and the rows are 16-byte aligned; None when the backward takes fp32 copies."""
    if not (MFMA16_WGRAD and ctx.mfma16 and x.dtype in _IO_CODE and g.dtype in (torch.float32, x.dtype) and
            (out is None or out.dtype == x.dtype) and
            _wgrad16_selects(x.shape[0], x.shape[2], x.shape[3], x.shape[1], weight.shape[0], weight.shape[2], ctx.stride, ctx.pads)):
        return None
    g = _dense_nhwc(g, any_dtype=True)
    return g if _rows_aligned(x, 16) and _rows_aligned(g, 16) else None


def _post_act_grad(g, out, slope, want_b, dt16):
    """Backward step 1, in one pass where a kernel has it: gp = g * LeakyReLU'(out) (g itself without an activation) and the bias
    gradient -> (gp, d_b or None).  fp32 operands (dt16 None): sr_act_bwd_bias_nhwc, or sr_act_bwd alone (FUSED_ACT_BIAS = 0,
    Cout % 4 != 0, no pixels: the caller then takes the bias gradient from gp).  16-bit operands: sr_act_bwd_bias16_nhwc, which
    also rounds an fp32 `g` to the layer's dtype `dt16`."""
    dev = g.device
    b, co, ho, wo = g.shape
    px = b * ho * wo
    act = slope is not None
    if dt16 is not None:
        write_gp = act or g.dtype != dt16
    elif FUSED_ACT_BIAS and co % 4 == 0 and b > 0:
        write_gp = act
    else:
        if not act:
            return g, None
        gp = torch.empty_like(g)
        _lib.call("sr_act_bwd", dev, g, _dense_nhwc(out), gp, g.numel(), float(slope))
        return gp, None
    if not (write_gp or want_b):
        return g, None
    gp = torch.empty_like(g, dtype=dt16 or torch.float32) if write_gp else g
    kernel = "sr_act_bwd_bias16" if dt16 is not None else "sr_act_bwd_bias"
    # (the bias gradient is a deterministic two-stage sum through a workspace)
    nws = getattr(_lib.lib(), kernel + "_workspace_bytes")(px, co) if want_b else 0
    ws = _workspace(dev, "bias_grad", nws) if want_b else None
    d_b = torch.empty((co,), dtype=torch.float32, device=dev) if want_b else None
    out = _dense_nhwc(out, any_dtype=dt16 is not None) if act else None
    tail = (gp if write_gp else None, d_b, px, co, float(slope) if act else 0.0)
    if dt16 is None:
        _lib.call("sr_act_bwd_bias_nhwc", dev, g, out, *tail, ws, nws)
    else:
        io = _IO_CODE[dt16]
        _lib.call("sr_act_bwd_bias16_nhwc", dev, g, 0 if g.dtype == torch.float32 else io, out, *tail, io, ws, nws)
    return gp, d_b


def _weight_grad(x, gp, weight, stride, pads):
    """Backward step 2: dL/dW as a dense fp32 [Co][Ci][k][k] tensor from the saved input and the post-activation gradient, both
    fp32 (sr_conv_wgrad_nhwc, or sr_conv_wgrad_padded_nhwc for explicit `pads`) or both 16-bit (sr_conv16_wgrad_nhwc)."""
    lib = _lib.lib()
    dev = x.device
    b, ci, h, w = x.shape
    co, _, k, _ = weight.shape
    ho, wo = gp.shape[2], gp.shape[3]
    if b == 0:
        return torch.zeros(weight.shape, dtype=torch.float32, device=dev)
    d_w = torch.empty(weight.shape, dtype=torch.float32, device=dev)   # (NOT empty_like: a channels_last weight's strides)
    head = (x, *_strides(x), gp, *_strides(gp), d_w, b, h, w, ci, co, k, stride)
    if x.dtype in _IO_CODE:
        nws = lib.sr_conv16_wgrad_workspace_bytes(b, h, w, ci, co, k, stride)
        _lib.call("sr_conv16_wgrad_nhwc", dev, *head, _IO_CODE[x.dtype], _workspace(dev, "wgrad", nws), nws)
    elif pads is None:
        nws = lib.sr_conv_wgrad_workspace_bytes(b, h, w, ci, co, k, stride)
        _lib.call("sr_conv_wgrad_nhwc", dev, *head, _workspace(dev, "wgrad", nws), nws)
    else:
        nws = lib.sr_conv_wgrad_padded_workspace_bytes(b, ho, wo, ci, co, k)
        _lib.call("sr_conv_wgrad_padded_nhwc", dev, *head, pads[0], pads[1], ho, wo, _workspace(dev, "wgrad", nws), nws)
    return d_w


def _data_grad(gp, weight, x_shape, stride, pads, dt16, out_f32):
    """Backward step 3: dL/dx = conv_s1(gp, flip(W)^T), at stride 2 on the zero-stuffed gp (the fp32 stuffing kernel, whatever gp's
    dtype).  `dt16`: the layer's dtype when its forward ran on the 16-bit MFMA kernel -- so does the data gradient, on the
    gradient cast to it, with d_x in fp32 when the caller's x was (`out_f32`: no cast behind the kernel)."""
    dev = gp.device
    b, ci, h, w = x_shape
    co, _, k, _ = weight.shape
    ho, wo = gp.shape[2], gp.shape[3]
    wt = torch.empty((ci, co, k, k), dtype=torch.float32, device=dev)
    _lib.call("sr_conv_flip_transpose_weights", dev, weight.detach().contiguous(), co, ci, k, wt)
    src = gp
    if stride != 1:   # the stuffed gradient lives on the input's H x W grid
        src = empty_nhwc(b, co, h, w, dev)
        if b > 0:
            g32 = gp.float()
            _lib.call("sr_zero_stuff2x_nhwc", dev, g32, *_strides(g32), src, b, ho, wo, h, w, co)
    if dt16 is not None and b > 0:
        src = src.to(dt16)
        if _conv16_routes(src, wt, 1, None, None):
            return _conv16(src, wt, None, 1, None, None, out_f32=out_f32)
        # (MFMA16 = 1 and the rule declines the transposed shape, or the switch changed since the forward)
    if pads is not None:   # full correlation: pads k-1-p on the opposite roles; stuffed: output H x W needs (k-1-pt, k-1-pl, pt, pl)
        pads = (k - 1 - pads[0], k - 1 - pads[1]) + ((k - 1 - pads[2], k - 1 - pads[3]) if stride == 1 else (pads[0], pads[1]))
    return _conv_raw(src, wt, None, 1, pads=pads)


class _ConvBiasAct(torch.autograd.Function):
    """y = act(conv(x, W, stride, pad = k // 2 or explicit `pads`) + b [+ residual]), act = LeakyReLU(slope) or identity
    (slope None).  `pads` = (top, left, bottom, right) zero padding (TF-"SAME" convolutions of the image-prior encoder,
    the valid convolution behind the matching encoder's replicate pad)."""

    @staticmethod
    @_amp_state_fwd
    def forward(ctx, x, weight, bias, residual, stride, slope, pads=None):
        # activation dtype of this layer: the autocast dtype with 16-bit kernel I/O, fp32 otherwise (inputs that arrive
        # in another floating dtype are cast: a differentiable cast, gradients go back in the caller's dtype)
        dt = ctx._sr_autocast_dtype if (ctx._sr_autocast and HALF_IO and ctx._sr_autocast_dtype in _IO_CODE) else torch.float32
        if not ctx._sr_autocast:   # outside autocast the path is fp32 only, loudly (as everywhere in this package)
            for name, t in (("conv input", x), ("conv weight", weight)) + ((("residual", residual),) if residual is not None else ()):
                _lib.require_device_f32(name, t)
        ctx.in_dtypes = (x.dtype, residual.dtype if residual is not None else None)
        x = x if x.dtype == dt else x.to(dt)
        if residual is not None and residual.dtype != dt:
            residual = residual.to(dt)
        weight = weight if weight.dtype == torch.float32 else weight.float()
        if bias is not None and bias.dtype != torch.float32:
            bias = bias.float()
        if dt == torch.float32:
            for name, t in (("conv input", x), ("conv weight", weight)):
                _lib.require_device_f32(name, t)
            x = as_nhwc(x, "conv input")
            ctx.mfma16 = False
            out = _conv_raw(x, weight, bias, stride, residual, slope, pads)
        else:   # whether the layer runs on the 16-bit MFMA kernel is decided here, once: the launch and the backward follow it
            x = _nhwc_any(x, "conv input")
            residual = _nhwc_any(residual, "residual") if residual is not None else None
            ctx.mfma16 = _conv16_routes(x, weight, stride, residual, pads)
            out = _conv_raw_io(x, weight, bias, stride, residual, slope, pads, mfma16=ctx.mfma16)
        ctx.stride, ctx.slope, ctx.pads = stride, slope, pads
        ctx.has_bias, ctx.has_res = bias is not None, residual is not None
        _stash(ctx, x, weight, out if slope is not None else None)
        return out

    @staticmethod
    @_amp_state_bwd
    def backward(ctx, g):
        x, weight, out = _unstash(ctx)
        dt16 = x.dtype if ctx.mfma16 else None   # the layer's 16-bit dtype when its forward ran on the 16-bit MFMA kernel
        g16 = _grad16(ctx, g, x, weight, out)
        if g16 is not None:
            g, op16 = g16, dt16
        else:   # the backward kernels take fp32 copies of what the forward saved in 16 bits
            x = x if x.dtype == torch.float32 else x.float()
            out = out if (out is None or out.dtype == torch.float32) else out.float()
            g, op16 = _dense_nhwc(g if g.dtype == torch.float32 else g.float()), None
        need_x, need_w, need_b, need_r = ctx.needs_input_grad[:4]
        want_b = ctx.has_bias and need_b
        d_x = d_w = None
        with _lib.on_device(x.device):
            gp, d_b = _post_act_grad(g, out, ctx.slope, want_b, op16)
            if need_w:
                d_w = _weight_grad(x, gp, weight, ctx.stride, ctx.pads)
            if want_b and d_b is None:   # (behind the unfused sr_act_bwd)
                d_b = torch.empty((weight.shape[0],), dtype=torch.float32, device=x.device)
                _lib.call("sr_bias_grad_nhwc", x.device, gp, *_strides(gp), d_b, g.shape[0], g.shape[2], g.shape[3], weight.shape[0])
            if need_x:
                d_x = _data_grad(gp, weight, x.shape, ctx.stride, ctx.pads, dt16, ctx.in_dtypes[0] == torch.float32)
        d_r = gp if (ctx.has_res and need_r) else None
        xdt, rdt = ctx.in_dtypes
        if d_x is not None and d_x.dtype != xdt:
            d_x = d_x.to(xdt)
        if d_r is not None and d_r.dtype != rdt:
            d_r = d_r.to(rdt)
        return d_x, d_w, d_b, d_r, None, None, None


class _Upsample2x(torch.autograd.Function):
    """Bilinear x2, align_corners=False (reference generic_utils.py:96-105) with its adjoint as backward."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, x):
        from . import ops
        with torch.no_grad():
            return ops.upsample2x(x.detach())

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        g = _dense_nhwc(g)
        b, c, h2, w2 = g.shape
        h, w = h2 // 2, w2 // 2
        out = empty_nhwc(b, c, h, w, g.device)
        if b > 0:
            gsb, gsp = _strides(g)
            osb, osp = _strides(out)
            _lib.call("sr_upsample2x_bwd_nhwc", g.device, g, gsb, gsp, out, osb, osp, b, h, w, c)
        return out


class _Exp(torch.autograd.Function):
    """depth = exp(log_depth) (reference depth_model.py:392-400); backward = grad * depth."""

    @staticmethod
    @_amp_fwd
    def forward(ctx, x):
        from . import ops
        with torch.no_grad():
            y = ops.exp(x.detach())
        ctx.save_for_backward(y)
        return y

    @staticmethod
    @_amp_bwd
    def backward(ctx, g):
        (y,) = ctx.saved_tensors
        g = g.contiguous() if y.is_contiguous() else g.contiguous(memory_format=torch.channels_last)
        if g.stride() != y.stride():
            g = g.contiguous()
            y = y.contiguous()
        out = torch.empty_like(y)
        _lib.call("sr_mul_fwd", y.device, g, y, out, y.numel())
        return out


def conv_bias_act(x, conv: nn.Conv2d, residual=None, slope=None):
    if conv.padding_mode != "zeros" or conv.groups != 1 or conv.dilation != (1, 1) or \
            tuple(conv.padding) != (conv.kernel_size[0] // 2,) * 2 or conv.kernel_size[0] not in (1, 3):
        raise _lib.HipLibraryError(f"unsupported Conv2d configuration for the HIP training path: {conv}")
    return _ConvBiasAct.apply(x, conv.weight, conv.bias, residual, conv.stride[0], slope)


def basic_block(block, x):
    """Differentiable BasicBlock.forward (reference layers.py:68-85), norm_layer = Identity."""
    if not isinstance(block.bn1, nn.Identity) or not isinstance(block.bn2, nn.Identity):
        raise _lib.HipLibraryError("the HIP BasicBlock implements norm_layer=nn.Identity only (what SimpleRecon uses)")
    slope = block.relu.negative_slope
    t = conv_bias_act(x, block.conv1, slope=slope)
    identity = x if block.downsample is None else conv_bias_act(x, block.downsample[0])
    return conv_bias_act(t, block.conv2, residual=identity, slope=slope)


def upsample2x(x):
    return _Upsample2x.apply(x)


def exp(x):
    return _Exp.apply(x)
