"""Frame preparation on HIP kernels (csrc/sr_frames.hip, csrc/sr_frames_jitter.hip): from a decoded frame -- an 8-bit
colour image, a 16-bit depth map, a pose and the depth sensor's intrinsics -- to the `cur_data` / `src_data`
dictionaries DepthModel and evaluate consume, with the bits the reference's loader produces
(datasets/generic_mvs_dataset.py get_frame, datasets/scannet_dataset.py load_intrinsics /
load_target_size_depth_and_mask, utils/generic_utils.py read_image_file).  The rules are stated in
include/simplerecon_hip.h, section "frame preparation".

    resample_tables(in_size, out_size, resample) -> (first, count, weights_i32)     host, Pillow's coefficient rules
    nearest_table(in_size, out_size) -> int32 source indices                        host, Pillow's nearest rule
    resize_u8(image_bhwc, height, width, resample="bilinear") -> uint8 [B,H,W,C]    Pillow's Image.resize
    prepare_color(image_bhwc, height, width, ...) -> fp32 [B,3,H,W]                 + to_tensor + ImageNet normalise
    prepare_depth(depth_bhw, height, width, ...) -> (depth_b1hw, mask_b1hw, mask_b_b1hw)
    scaled_intrinsics(K_44, ...) -> {K_s{i}_b44, invK_s{i}_b44, ...}                host, the reference's operations
    jitter_params(n, 0.2, 0.2, 0.2, 0.2, generator=None) -> JitterParams             host, ColorJitter's draws per frame
    JitterParams.from_values(order, brightness, contrast, saturation, hue)          host, explicit values (None = off)
    prepare_color_jittered(image_bhwc, height, width, params, ...) -> fp32 [B,3,H,W]   resize + ColorJitter + flip + normalise
    FramePreparer(...).frame(...) / .tuple(frames) -> get_frame's dictionary / (cur_data, src_data)
    FramePreparer(color_jitter=(0.2, 0.2, 0.2, 0.2)).train_tuple(frames) -> the training split's tuple: random flip + jitter

The colour jitter restates torchvision's published tensor path (the package is not a dependency and was absent where
this was written): parity against the package itself is unpinned.  tests/jitter_oracle.py is the rule in torch's CPU
operations; the kernels follow it within a few fp32 roundings (the mean of contrast is summed in another order).

Out of scope:
  - reading and decoding image files (PNG / JPEG decoding stays on the host);
  - torchvision's PIL path, its other transforms, and jitter of fp32 images that did not come from 8-bit ones;
  - the per-dataset path and metadata conventions (which file holds the pose, the intrinsics, the depth size);
  - crop_image_to_target_ratio: the reference discards its result, so there it does nothing.
A four-channel image is resized channel by channel (Pillow's CMYK / RGBX); Pillow premultiplies RGBA, this does not.
Depth values are float(v) * scale for v in 0..65535 whatever the input dtype.

There is no CPU path: with no GPU visible every entry point that launches raises HipLibraryError.  numpy arrays and
host tensors are accepted as a convenience and copied to the device once."""
import math

import numpy as np
import torch

from . import _lib
from .keyframes import sort_sources_by_pose_penalty

TILE_W, TILE_H = 128, 16      # SR_FRAMES_TILE_W, SR_FRAMES_TILE_H
MAX_SIDE = 32768              # SR_FRAMES_MAX_SIDE
MAX_BATCH = 65535             # SR_FRAMES_MAX_BATCH
PRECISION_BITS = 22           # Pillow's fixed point for 8-bit channels
IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)

# Which of the two colour paths the last resize_u8 / prepare_color calls took: "fused" (one launch, rows in LDS) or
# "two_pass" (through a uint8 intermediate).  Counters for tests and profiling; the results do not depend on the path.
path_counts = {"fused": 0, "two_pass": 0}


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


FILTERS = {"bilinear": (_bilinear, 1.0), "box": (_box, 0.5), "hamming": (_hamming, 1.0), "bicubic": (_bicubic, 2.0),
           "lanczos": (_lanczos, 3.0)}


def _check_sizes(**sizes):
    out = []
    for name, v in sizes.items():
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"{name} must be an int, got {type(v)}")
        if not 1 <= int(v) <= MAX_SIDE:
            raise ValueError(f"{name} must be in [1, {MAX_SIDE}], got {v}")
        out.append(int(v))
    return out


def resample_tables(in_size, out_size, resample="bilinear"):
    """Pillow's resampling coefficients for one pass over 8-bit channels from `in_size` to `out_size` samples:
    (first [out] int32, count [out] int32, weights [out, taps] int32 in 2^22 fixed point, zero past count).  Output i
    is clamp((2^21 + sum_k weights[i, k] * v[first[i] + k]) >> 22, 0, 255).  in_size == out_size gives the identity
    (one tap of weight 2^22), which is what Pillow's skipped pass amounts to.

    resample: "bilinear", "bicubic", "lanczos", "box" or "hamming".  All five are built: each is checked bit for bit
    against Pillow's Image.resize by the fixtures of tests/golden/make_frames_golden.py."""
    if resample not in FILTERS:
        raise ValueError(f"resample must be one of {sorted(FILTERS)}, got {resample!r}")
    n_in, n_out = _check_sizes(in_size=in_size, out_size=out_size)
    if n_in == n_out:
        return (np.arange(n_out, dtype=np.int32), np.ones(n_out, dtype=np.int32),
                np.full((n_out, 1), 1 << PRECISION_BITS, dtype=np.int32))
    filt, filter_support = FILTERS[resample]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = filter_support * fs
    ss = 1.0 / fs
    first = np.empty(n_out, dtype=np.int32)
    count = np.empty(n_out, dtype=np.int32)
    rows = []
    for i in range(n_out):
        center = (i + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), n_in)
        w = [filt((x + lo - center + 0.5) * ss) for x in range(hi - lo)]
        total = 0.0
        for v in w:
            total += v
        if total != 0.0:
            w = [v / total for v in w]
        first[i], count[i] = lo, hi - lo
        rows.append([int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w])
    taps = max(1, int(count.max()))
    weights = np.zeros((n_out, taps), dtype=np.int32)
    for i, r in enumerate(rows):
        weights[i, :len(r)] = r
    return first, count, weights


def nearest_table(in_size, out_size):
    """Source index of every output sample of Pillow's NEAREST resize: floor((i + 0.5) * in / out) in double."""
    n_in, n_out = _check_sizes(in_size=in_size, out_size=out_size)
    scale = n_in / n_out
    return np.array([min(int((i + 0.5) * scale), n_in - 1) for i in range(n_out)], dtype=np.int32)


def rows_needed(first, count, tile=TILE_H):
    """The largest number of input rows any `tile` consecutive output rows tap: what the fused kernel keeps in LDS."""
    n = len(first)
    last = first.astype(np.int64) + count
    return max(int(last[y0:y0 + tile].max() - first[y0:y0 + tile].min()) for y0 in range(0, n, tile))


# ---- device-side caches: filled on the first call for a key, read without a copy or a synchronisation afterwards ----
_TABLES = {}    # (device, in, out, resample) -> (packed int32 table, taps, rows_needed)
_NEAREST = {}   # (device, in, out) -> int32 indices
_LUT = {}       # (device, channels) -> fp32 [C, 256]


def _packed_table(dev, n_in, n_out, resample):
    key = (dev, n_in, n_out, resample)
    hit = _TABLES.get(key)
    if hit is None:
        first, count, weights = resample_tables(n_in, n_out, resample)
        packed = np.concatenate([first[:, None], count[:, None], weights], axis=1).astype(np.int32)
        hit = _TABLES[key] = (torch.from_numpy(np.ascontiguousarray(packed)).to(dev), int(weights.shape[1]),
                              rows_needed(first, count))
    return hit


def _nearest(dev, n_in, n_out):
    key = (dev, n_in, n_out)
    hit = _NEAREST.get(key)
    if hit is None:
        hit = _NEAREST[key] = torch.from_numpy(nearest_table(n_in, n_out)).to(dev)
    return hit


def normalise_table():
    """fp32 [3, 256]: ((v / 255) - mean_c) / std_c with torch's CPU kernels -- to_tensor's division, then
    TF.normalize's sub_ and div_ -- so the device result has their rounding."""
    v = torch.arange(256, dtype=torch.float32).div(255)
    mean = torch.tensor(IMAGENET_MEAN, dtype=torch.float32)[:, None]
    std = torch.tensor(IMAGENET_STD, dtype=torch.float32)[:, None]
    return v[None].repeat(3, 1).sub_(mean).div_(std).contiguous()


def _lut(dev):
    hit = _LUT.get(dev)
    if hit is None:
        hit = _LUT[dev] = normalise_table().to(dev)
    return hit


def _device(device=None):
    if not _lib.cuda_available():
        raise _lib.HipLibraryError("frame preparation runs on the GPU only and no GPU is visible (no CPU fallback)")
    if device is None:
        return torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    if dev.type != "cuda":
        raise _lib.HipLibraryError(f"frame preparation runs on the GPU only, got device {dev} (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)


def _to_device(name, a, dtypes, device):
    """A device tensor of one of `dtypes` (torch dtypes) from a device tensor, a host tensor or a numpy array."""
    if isinstance(a, np.ndarray):
        if a.dtype not in (np.uint8, np.uint16, np.int32):
            raise TypeError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got numpy {a.dtype}")
        a = torch.from_numpy(np.ascontiguousarray(a))
    if not isinstance(a, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor or a numpy array, got {type(a)}")
    if a.dtype not in dtypes:
        raise TypeError(f"{name} must be {' or '.join(str(d) for d in dtypes)}, got {a.dtype}")
    if not a.is_cuda:
        a = a.to(_device(device))
    elif device is not None and a.device != _device(device):
        raise ValueError(f"{name} on {a.device}, expected {_device(device)}")
    return a.detach().contiguous()


def _resize(image_bhwc, height, width, resample, flip, f32, device=None):
    H, W = _check_sizes(height=height, width=width)
    if resample not in FILTERS:
        raise ValueError(f"resample must be one of {sorted(FILTERS)}, got {resample!r}")
    if isinstance(image_bhwc, (np.ndarray, torch.Tensor)) and image_bhwc.ndim != 4:
        raise ValueError(f"image_bhwc must be [B,h,w,C], got {tuple(image_bhwc.shape)}")
    img = _to_device("image_bhwc", image_bhwc, (torch.uint8,), device)
    B, h, w, C = (int(s) for s in img.shape)
    if (C != 3) if f32 else not 1 <= C <= 4:
        raise ValueError(f"image_bhwc must have {'3 channels' if f32 else '1 to 4 channels'}, got {C}")
    if not 1 <= B <= MAX_BATCH:
        raise ValueError(f"the batch must be in [1, {MAX_BATCH}], got {B}")
    _check_sizes(input_height=h, input_width=w)
    dev = img.device
    with _lib.on_device(dev):
        xtab, xk, _ = _packed_table(dev, w, W, resample)
        ytab, yk, need = _packed_table(dev, h, H, resample)
        lut = _lut(dev) if f32 else None
        out = torch.empty((B, C, H, W), dtype=torch.float32, device=dev) if f32 else \
            torch.empty((B, H, W, C), dtype=torch.uint8, device=dev)
        fused = bool(_lib.lib().sr_frames_resize_fits_lds(C, xk, need, int(f32)))
        tmp = None if fused else torch.empty((B, h, W, C), dtype=torch.uint8, device=dev)
        _lib.call("sr_frames_resize", dev, img, B, h, w, C, xtab, xk, ytab, yk, need if fused else 0, lut, out, int(f32),
                  H, W, int(bool(flip)), tmp)
    path_counts["fused" if fused else "two_pass"] += 1
    return out


def resize_u8(image_bhwc, height, width, resample="bilinear"):
    """Pillow's Image.resize((width, height), resample) of B interleaved 8-bit images [B,h,w,C], C in 1..4:
    uint8 [B,H,W,C] on the device, every byte equal to Pillow's."""
    return _resize(image_bhwc, height, width, resample, False, False)


def prepare_color(image_bhwc, height, width, resample="bilinear", flip=False):
    """The model's colour input from B decoded RGB images uint8 [B,h,w,3]: Pillow's resize, to_tensor, the optional
    x-flip and ImageNet normalisation in one launch.  fp32 [B,3,H,W] with the bits of the reference's CPU loader."""
    return _resize(image_bhwc, height, width, resample, flip, True)


JITTER_OPS = ("brightness", "contrast", "saturation", "hue")   # SR_FRAMES_JITTER_*: the ids of an operator order
JITTER_WORDS = 12                                              # SR_FRAMES_JITTER_PARAM_WORDS
_NEUTRAL = (1.0, 1.0, 1.0, 0.0)


def jitter_range(name, value):
    """ColorJitter's range of one argument (its _check_input): a number a gives [max(0, 1 - a), 1 + a], for hue
    [-a, a] with 0 <= a <= 0.5; a (lo, hi) pair is taken as given; None, or a range that collapses to the neutral
    value, switches the operator off.  Returns (lo, hi) or None."""
    if name not in JITTER_OPS:
        raise ValueError(f"name must be one of {JITTER_OPS}, got {name!r}")
    if value is None:
        return None
    hue = name == "hue"
    center, lo_bound, hi_bound = (0.0, -0.5, 0.5) if hue else (1.0, 0.0, math.inf)
    if isinstance(value, (int, float, np.integer, np.floating)) and not isinstance(value, bool):
        if value < 0:
            raise ValueError(f"if {name} is a single number, it must be non negative")
        lo, hi = center - float(value), center + float(value)
        if not hue:
            lo = max(lo, 0.0)
    elif isinstance(value, (tuple, list)) and len(value) == 2:
        lo, hi = float(value[0]), float(value[1])
    else:
        raise TypeError(f"{name} should be a single number or a list/tuple with length 2")
    if not lo_bound <= lo <= hi <= hi_bound:
        raise ValueError(f"{name} values should be between ({lo_bound}, {hi_bound}), got ({lo}, {hi})")
    return None if lo == hi == center else (lo, hi)


class JitterParams:
    """The colour jitter of n frames: `order` int64 [n,4], the operator ids (0 brightness, 1 contrast, 2 saturation,
    3 hue) in the order they run; `factors` float64 [n,4], indexed by operator id; `on`, four booleans, which
    operators run at all (one answer for all frames, as ColorJitter's).  An operator that is off keeps its neutral
    factor and is left out of the order the kernels see."""

    def __init__(self, order, factors, on):
        self.order = np.ascontiguousarray(order, dtype=np.int64)
        self.factors = np.ascontiguousarray(factors, dtype=np.float64)
        self.on = tuple(bool(v) for v in on)
        if self.order.ndim != 2 or self.order.shape[1] != 4 or self.factors.shape != self.order.shape or \
                len(self.on) != 4:
            raise ValueError(f"order and factors must be [n,4] and `on` four booleans, got {self.order.shape}, "
                             f"{self.factors.shape}, {len(self.on)}")
        if (np.sort(self.order, axis=1) != np.arange(4)).any():
            raise ValueError("every row of order must be a permutation of 0, 1, 2, 3")
        if not np.isfinite(self.factors).all():
            raise ValueError("the factors must be finite")
        if (self.factors[:, :3] < 0).any() or (np.abs(self.factors[:, 3]) > 0.5).any():
            raise ValueError("brightness, contrast and saturation factors are non-negative, a hue shift lies in "
                             "[-0.5, 0.5]")

    def __len__(self):
        return int(self.order.shape[0])

    @classmethod
    def from_values(cls, order, brightness=None, contrast=None, saturation=None, hue=None):
        """Explicit values: `order` [4] or [n,4]; each factor a number, n numbers, or None = that operator is off."""
        order = np.asarray(order, dtype=np.int64)
        order = order[None] if order.ndim == 1 else order
        values = (brightness, contrast, saturation, hue)
        n = max([order.shape[0]] + [np.size(v) for v in values if v is not None])
        if order.ndim != 2 or order.shape[0] not in (1, n):
            raise ValueError(f"order must be [4] or [{n},4], got {order.shape}")
        factors = np.empty((n, 4), dtype=np.float64)
        for k, v in enumerate(values):
            v = np.asarray(_NEUTRAL[k] if v is None else v, dtype=np.float64).reshape(-1)
            if v.size not in (1, n):
                raise ValueError(f"{JITTER_OPS[k]}: {v.size} values for {n} frames")
            factors[:, k] = v
        return cls(np.broadcast_to(order, (n, 4)), factors, [v is not None for v in values])

    def table(self):
        """The kernels' table, int32 [n, 12] (include/simplerecon_hip.h): the operators that are on in the order they
        run, -1 in the empty slots, then the bits of (f, 1 - f) of brightness, contrast and saturation and of the hue
        shift.  1 - f is computed in double and both are rounded to fp32, as torch rounds a Python scalar."""
        n = len(self)
        slots = np.full((n, 4), -1, dtype=np.int32)
        for i in range(n):
            ops = [int(o) for o in self.order[i] if self.on[o]]
            slots[i, :len(ops)] = ops
        f = np.zeros((n, 8), dtype=np.float32)
        for k in range(3):
            f[:, 2 * k] = self.factors[:, k]
            f[:, 2 * k + 1] = 1.0 - self.factors[:, k]
        f[:, 6] = self.factors[:, 3]
        return np.ascontiguousarray(np.concatenate([slots, f.view(np.int32)], axis=1))


def jitter_params(n, brightness=0.2, contrast=0.2, saturation=0.2, hue=0.2, generator=None):
    """ColorJitter(brightness, contrast, saturation, hue).get_params, once per frame for n frames, from torch's global
    generator or from `generator`: per frame torch.randperm(4), then, for each operator that is on, in the order
    brightness, contrast, saturation, hue, float(torch.empty(1).uniform_(lo, hi)).  An operator that is off draws
    nothing."""
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or n < 1:
        raise ValueError(f"n must be a positive int, got {n!r}")
    ranges = [jitter_range(name, v) for name, v in zip(JITTER_OPS, (brightness, contrast, saturation, hue))]
    order = np.empty((n, 4), dtype=np.int64)
    factors = np.tile(np.array(_NEUTRAL, dtype=np.float64), (n, 1))
    for i in range(n):
        order[i] = torch.randperm(4, generator=generator).numpy()
        for k, r in enumerate(ranges):
            if r is not None:
                factors[i, k] = float(torch.empty(1).uniform_(r[0], r[1], generator=generator))
    return JitterParams(order, factors, [r is not None for r in ranges])


def prepare_color_jittered(image_bhwc, height, width, params, resample="bilinear", flip=False, normalize=True):
    """prepare_color with the training split's augmentation: Pillow's resize, to_tensor, ColorJitter with frame i's
    `params` (a JitterParams of B frames), the optional x-flip, the ImageNet normalisation unless normalize=False.
    fp32 [B,3,H,W].  The resize launch, then two for the whole batch (one when no frame has contrast on); the table
    goes to the device in one copy.  With every operator off, or all factors neutral, the bytes of prepare_color."""
    if not isinstance(params, JitterParams):
        raise TypeError(f"params must be a JitterParams, got {type(params)}")
    small = resize_u8(image_bhwc, height, width, resample)
    B, H, W, C = (int(v) for v in small.shape)
    if C != 3:
        raise ValueError(f"image_bhwc must have 3 channels, got {C}")
    if len(params) != B:
        raise ValueError(f"params holds {len(params)} frames, the batch {B}")
    table = params.table()
    _lib.check(_lib.lib().sr_frames_jitter_check_params(table.ctypes.data, B), "sr_frames_jitter_check_params")
    dev = small.device
    with _lib.on_device(dev):
        table_dev = torch.from_numpy(table).to(dev)
        nbytes = int(_lib.lib().sr_frames_jitter_scratch_bytes(B, H, W)) if params.on[1] else 0
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev) if nbytes else None
        out = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
        _lib.call("sr_frames_jitter", dev, small, B, H, W, table_dev, out, int(bool(flip)), int(bool(normalize)), scratch,
                  nbytes)
    return out


def prepare_depth(depth_bhw, height=None, width=None, scale=1e-3, min_valid=1e-3, max_valid=10.0, flip=False):
    """The reference's depth loading for B sensor depth maps [B,h,w] (uint16 or int32, values 0..65535): Pillow's
    nearest resize to height x width (None: the native size), depth = float(v) * scale, valid where
    min_valid < depth < max_valid, NaN elsewhere.  Returns (depth_b1hw fp32, mask_b1hw fp32, mask_b_b1hw bool)."""
    if (height is None) != (width is None):
        raise ValueError("height and width are given together or not at all")
    if isinstance(depth_bhw, (np.ndarray, torch.Tensor)) and depth_bhw.ndim != 3:
        raise ValueError(f"depth_bhw must be [B,h,w], got {tuple(depth_bhw.shape)}")
    d = _to_device("depth_bhw", depth_bhw, (torch.uint16, torch.int32), None)
    B, h, w = (int(s) for s in d.shape)
    _check_sizes(input_height=h, input_width=w)
    H, W = (h, w) if height is None else _check_sizes(height=height, width=width)
    if not 1 <= B <= MAX_BATCH:
        raise ValueError(f"the batch must be in [1, {MAX_BATCH}], got {B}")
    dev = d.device
    with _lib.on_device(dev):
        ysrc, xsrc = _nearest(dev, h, H), _nearest(dev, w, W)
        depth = torch.empty((B, 1, H, W), dtype=torch.float32, device=dev)
        mask = torch.empty_like(depth)
        mask_b = torch.empty((B, 1, H, W), dtype=torch.bool, device=dev)
        _lib.call("sr_frames_depth", dev, d, int(d.dtype == torch.int32), B, h, w, ysrc, xsrc, H, W, float(scale),
                  float(min_valid), float(max_valid), int(bool(flip)), depth, mask, mask_b)
    return depth, mask, mask_b


def scaled_intrinsics(K_44, native_width, native_height, depth_width, depth_height, flip=False,
                      include_full_depth_K=False):
    """The reference's intrinsics dictionary (scannet_dataset.py:450-470) from the depth sensor's 4x4 intrinsics at its
    native width x height: K_s{i}_b44 / invK_s{i}_b44 for i in 0..4, scale 0 at depth_width x depth_height and each
    further scale half of the one before; K_full_depth_b44 / invK_full_depth_b44 when asked.  With flip the principal
    point is mirrored (cx = native_width - cx) first.  Host fp32 tensors [4,4], computed with the reference's own
    operations (in-place fp32 row scaling, a LAPACK fp32 inverse per scale), so equal to it bit for bit."""
    K = torch.tensor(np.asarray(K_44.detach().cpu() if isinstance(K_44, torch.Tensor) else K_44).astype(np.float32))
    if tuple(K.shape) != (4, 4):
        raise ValueError(f"K_44 must be 4x4, got {tuple(K.shape)}")
    _check_sizes(native_width=native_width, native_height=native_height, depth_width=depth_width,
                 depth_height=depth_height)
    out = {}
    if flip:
        K[0, 2] = float(native_width) - K[0, 2]
    if include_full_depth_K:
        out["K_full_depth_b44"] = K.clone()
        out["invK_full_depth_b44"] = torch.tensor(np.linalg.inv(K.numpy()))
    K[0] *= depth_width / float(native_width)
    K[1] *= depth_height / float(native_height)
    for i in range(5):
        K_scaled = K.clone()
        K_scaled[:2] /= 2 ** i
        out[f"K_s{i}_b44"] = K_scaled
        out[f"invK_s{i}_b44"] = torch.tensor(np.linalg.inv(K_scaled.numpy()))
    return out


def flipped_pose(world_T_cam_44, flip=False):
    """(world_T_cam, cam_T_world) as fp32 numpy 4x4 the way the reference loads a pose (scannet_dataset.py:565-566),
    mirrored along x when flip (generic_mvs_dataset.py:508-512)."""
    pose = np.asarray(world_T_cam_44.detach().cpu() if isinstance(world_T_cam_44, torch.Tensor)
                      else world_T_cam_44).astype(np.float32)
    if pose.shape != (4, 4):
        raise ValueError(f"world_T_cam_44 must be 4x4, got {pose.shape}")
    if flip:
        T = np.eye(4).astype(pose.dtype)
        T[0, 0] = -1.0
        pose = pose @ T
    return pose, np.linalg.inv(pose)


class FramePreparer:
    """GenericMVSDataset.get_frame / __getitem__ without the files: decoded frames in, the reference's dictionaries
    out, tensors on the device.  The constructor arguments are the dataset's."""

    def __init__(self, image_height=384, image_width=512, depth_height=192, depth_width=256, high_res_image_height=480,
                 high_res_image_width=640, include_high_res_color=False, include_full_res_depth=False,
                 include_full_depth_K=False, min_valid_depth=1e-3, max_valid_depth=10.0, resample="bilinear",
                 device=None, color_jitter=None):
        _check_sizes(image_height=image_height, image_width=image_width, depth_height=depth_height,
                     depth_width=depth_width, high_res_image_height=high_res_image_height,
                     high_res_image_width=high_res_image_width)
        if resample not in FILTERS:
            raise ValueError(f"resample must be one of {sorted(FILTERS)}, got {resample!r}")
        self.image_height, self.image_width = int(image_height), int(image_width)
        self.depth_height, self.depth_width = int(depth_height), int(depth_width)
        self.high_res_image_height, self.high_res_image_width = int(high_res_image_height), int(high_res_image_width)
        self.include_high_res_color = bool(include_high_res_color)
        self.include_full_res_depth = bool(include_full_res_depth)
        self.include_full_depth_K = bool(include_full_depth_K)
        self.min_valid_depth, self.max_valid_depth = float(min_valid_depth), float(max_valid_depth)
        self.resample = resample
        self.device = device
        # the dataset's color_transform: None, or ColorJitter's four arguments (brightness, contrast, saturation, hue)
        if color_jitter is not None:
            color_jitter = tuple(color_jitter)
            if len(color_jitter) != 4:
                raise ValueError("color_jitter is None or (brightness, contrast, saturation, hue)")
            for name, v in zip(JITTER_OPS, color_jitter):
                jitter_range(name, v)
        self.color_jitter = color_jitter

    def _batch(self, name, items, dtypes, ndim, dev):
        """One device tensor [N, ...] from N same-sized images (a single copy when they come from the host)."""
        for a in items:
            if not isinstance(a, (np.ndarray, torch.Tensor)):
                raise TypeError(f"{name} must be a torch.Tensor or a numpy array, got {type(a)}")
            if a.ndim != ndim:
                raise ValueError(f"{name} must have {ndim} dimensions, got shape {tuple(a.shape)}")
            if tuple(a.shape) != tuple(items[0].shape):
                raise ValueError(f"the frames of a tuple share one size: {name} {tuple(a.shape)} next to "
                                 f"{tuple(items[0].shape)}")
        if all(isinstance(a, np.ndarray) for a in items):
            return _to_device(name, np.stack(items), dtypes, dev)
        parts = [_to_device(name, a, dtypes, dev) for a in items]
        if parts[0].dtype == torch.uint16:     # (torch stacks the same bytes as int16: few kernels know uint16)
            return torch.stack([t.view(torch.int16) for t in parts]).view(torch.uint16)
        return torch.stack(parts)

    def _prepare(self, frames, flip, native_depth_size=None, jitter=None):
        """get_frame for N frames [(color, depth or None, world_T_cam, K_depth_native, frame_id_string or None)]:
        the images of all N go through one launch per output, the 4x4 matrices through the host.  jitter: a
        JitterParams of N frames for image_b3hw (get_frame's color_transform), or None."""
        if jitter is not None and not isinstance(jitter, JitterParams):
            raise TypeError(f"jitter must be a JitterParams or None, got {type(jitter)}")
        if jitter is not None and len(jitter) != len(frames):
            raise ValueError(f"jitter holds {len(jitter)} frames, the call {len(frames)}")
        dev = _device(self.device)
        flip = bool(flip)
        colors = self._batch("color_u8_hwc", [f[0] for f in frames], (torch.uint8,), 3, dev)
        have_depth = [f[1] is not None for f in frames]
        if any(have_depth) != all(have_depth):
            raise ValueError("the frames of a tuple come all with depth or all without")
        out = [{} for _ in frames]
        image = prepare_color(colors, self.image_height, self.image_width, self.resample, flip) if jitter is None else \
            prepare_color_jittered(colors, self.image_height, self.image_width, jitter, self.resample, flip)
        high = prepare_color(colors, self.high_res_image_height, self.high_res_image_width, self.resample,
                             flip) if self.include_high_res_color else None
        target = full = None
        if all(have_depth):
            depths = self._batch("depth_u16_hw", [f[1] for f in frames], (torch.uint16, torch.int32), 2, dev)
            native_h, native_w = int(depths.shape[1]), int(depths.shape[2])
            target = prepare_depth(depths, self.depth_height, self.depth_width, 1e-3, self.min_valid_depth,
                                   self.max_valid_depth, flip)
            if self.include_full_res_depth:
                full = prepare_depth(depths, None, None, 1e-3, self.min_valid_depth, self.max_valid_depth, flip)
        elif self.include_full_res_depth:
            raise ValueError("include_full_res_depth needs depth maps")
        elif native_depth_size is None:
            raise ValueError("without a depth map, native_depth_size=(height, width) says what size "
                             "K_depth_native_44 belongs to")
        else:
            native_h, native_w = native_depth_size
        poses = [flipped_pose(f[2], flip) for f in frames]
        intrinsics = [scaled_intrinsics(f[3], native_w, native_h, self.depth_width, self.depth_height, flip,
                                        self.include_full_depth_K) for f in frames]
        # every small matrix of the tuple in one host-to-device copy
        names = ["world_T_cam_b44", "cam_T_world_b44"] + list(intrinsics[0])
        host = torch.stack([torch.stack([torch.from_numpy(p[0]), torch.from_numpy(p[1])] + [k[n] for n in names[2:]])
                            for p, k in zip(poses, intrinsics)]).to(dev)
        for i, d in enumerate(out):
            d["image_b3hw"] = image[i]
            d["world_T_cam_b44"], d["cam_T_world_b44"] = host[i, 0], host[i, 1]
            for j, n in enumerate(names[2:]):
                d[n] = host[i, 2 + j]
            if target is not None:
                d["depth_b1hw"], d["mask_b1hw"], d["mask_b_b1hw"] = (t[i] for t in target)
            if high is not None:
                d["high_res_color_b3hw"] = high[i]
            if full is not None:
                d["full_res_depth_b1hw"], d["full_res_mask_b1hw"], d["full_res_mask_b_b1hw"] = (t[i] for t in full)
            if frames[i][4] is not None:
                d["frame_id_string"] = frames[i][4]
        return out, [p[0] for p in poses], [p[1] for p in poses]

    @staticmethod
    def _as_frame(f):
        f = tuple(f)
        if not 4 <= len(f) <= 5:
            raise ValueError("a frame is (color_u8_hwc, depth_u16_hw, world_T_cam_44, K_depth_native_44"
                             "[, frame_id_string])")
        return f if len(f) == 5 else f + (None,)

    def frame(self, color_u8_hwc, depth_u16_hw, world_T_cam_44, K_depth_native_44, flip=False, frame_id_string=None,
              native_depth_size=None, jitter=None):
        """One get_frame dictionary (no batch dimension; tensors on the device): image_b3hw, world_T_cam_b44,
        cam_T_world_b44, K_s{i}_b44 / invK_s{i}_b44, depth_b1hw, mask_b1hw, mask_b_b1hw, and what the include_*
        options add.  color_u8_hwc uint8 [h,w,3]; depth_u16_hw uint16 / int32 [h',w'] in millimetres;
        K_depth_native_44 the intrinsics at the depth map's native size.  depth_u16_hw may be None (get_frame's
        load_depth=False: no depth keys); native_depth_size=(height, width) then gives that size.  jitter: a
        JitterParams of one frame, the colour jitter of image_b3hw (no other key changes), or None."""
        out, _, _ = self._prepare([(color_u8_hwc, depth_u16_hw, world_T_cam_44, K_depth_native_44, frame_id_string)],
                                  flip, native_depth_size, jitter)
        return out[0]

    def tuple(self, frames, flip=False, native_depth_size=None, jitter=None):
        """(cur_data, src_data) of one MVS tuple from a list of frames, the reference frame first, each
        (color_u8_hwc, depth_u16_hw, world_T_cam_44, K_depth_native_44[, frame_id_string]).  src_data stacks the
        sources along a first dimension, ordered by the reference's pose penalty with respect to the reference frame
        (generic_mvs_dataset.py:643-659).  jitter: a JitterParams with one entry per frame, in the order of `frames`:
        the colour jitter of every image_b3hw (high_res_color_b3hw is never jittered), or None."""
        frames = [self._as_frame(f) for f in frames]
        if len(frames) < 2:
            raise ValueError("a tuple needs the reference frame and at least one source frame")
        out, world_T_cam, cam_T_world = self._prepare(frames, flip, native_depth_size, jitter)
        order = sort_sources_by_pose_penalty(cam_T_world[0], np.stack(world_T_cam[1:]))
        src = [out[1 + i] for i in order]
        src_data = {k: [s[k] for s in src] if k == "frame_id_string" else torch.stack([s[k] for s in src])
                    for k in src[0]}
        return out[0], src_data

    def train_tuple(self, frames, generator=None, native_depth_size=None):
        """tuple() as the training split draws it (generic_mvs_dataset.py:613-634, 517-519): the flip first, once for
        the tuple (torch.rand(1).item() < 0.5), then, with color_jitter set, the jitter of each frame in the order of
        `frames`, the reference frame first.  Draws from torch's global generator or from `generator`."""
        frames = list(frames)
        flip = torch.rand(1, generator=generator).item() < 0.5
        jitter = None if self.color_jitter is None else jitter_params(len(frames), *self.color_jitter,
                                                                      generator=generator)
        return self.tuple(frames, flip=flip, native_depth_size=native_depth_size, jitter=jitter)
