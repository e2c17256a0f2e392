"""Frame preparation on HIP kernels (csrc/sr_frames.hip): from a decoded frame -- an 8-bit colour image, a 16-bit
depth map, a pose and the depth sensor's intrinsics -- to the `cur_data` / `src_data` dictionaries DepthModel and
evaluate consume, with the bits the reference's loader produces (datasets/generic_mvs_dataset.py get_frame,
datasets/scannet_dataset.py load_intrinsics / load_target_size_depth_and_mask, utils/generic_utils.py
read_image_file).  The rules are stated in include/simplerecon_hip.h, section "frame preparation".

    resample_tables(in_size, out_size, resample) -> (first, count, weights_i32)     host, Pillow's coefficient rules
    nearest_table(in_size, out_size) -> int32 source indices                        host, Pillow's nearest rule
    resize_u8(image_bhwc, height, width, resample="bilinear") -> uint8 [B,H,W,C]    Pillow's Image.resize
    prepare_color(image_bhwc, height, width, ...) -> fp32 [B,3,H,W]                 + to_tensor + ImageNet normalise
    prepare_depth(depth_bhw, height, width, ...) -> (depth_b1hw, mask_b1hw, mask_b_b1hw)
    scaled_intrinsics(K_44, ...) -> {K_s{i}_b44, invK_s{i}_b44, ...}                host, the reference's operations
    FramePreparer(...).frame(...) / .tuple(frames) -> get_frame's dictionary / (cur_data, src_data)

Out of scope:
  - reading and decoding image files (PNG / JPEG decoding stays on the host);
  - ColorJitter, torchvision's random training augmentation;
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
                 device=None):
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

    def _prepare(self, frames, flip, native_depth_size=None):
        """get_frame for N frames [(color, depth or None, world_T_cam, K_depth_native, frame_id_string or None)]:
        the images of all N go through one launch per output, the 4x4 matrices through the host."""
        dev = _device(self.device)
        flip = bool(flip)
        colors = self._batch("color_u8_hwc", [f[0] for f in frames], (torch.uint8,), 3, dev)
        have_depth = [f[1] is not None for f in frames]
        if any(have_depth) != all(have_depth):
            raise ValueError("the frames of a tuple come all with depth or all without")
        out = [{} for _ in frames]
        image = prepare_color(colors, self.image_height, self.image_width, self.resample, flip)
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
              native_depth_size=None):
        """One get_frame dictionary (no batch dimension; tensors on the device): image_b3hw, world_T_cam_b44,
        cam_T_world_b44, K_s{i}_b44 / invK_s{i}_b44, depth_b1hw, mask_b1hw, mask_b_b1hw, and what the include_*
        options add.  color_u8_hwc uint8 [h,w,3]; depth_u16_hw uint16 / int32 [h',w'] in millimetres;
        K_depth_native_44 the intrinsics at the depth map's native size.  depth_u16_hw may be None (get_frame's
        load_depth=False: no depth keys); native_depth_size=(height, width) then gives that size."""
        out, _, _ = self._prepare([(color_u8_hwc, depth_u16_hw, world_T_cam_44, K_depth_native_44, frame_id_string)],
                                  flip, native_depth_size)
        return out[0]

    def tuple(self, frames, flip=False, native_depth_size=None):
        """(cur_data, src_data) of one MVS tuple from a list of frames, the reference frame first, each
        (color_u8_hwc, depth_u16_hw, world_T_cam_44, K_depth_native_44[, frame_id_string]).  src_data stacks the
        sources along a first dimension, ordered by the reference's pose penalty with respect to the reference frame
        (generic_mvs_dataset.py:643-659)."""
        frames = [self._as_frame(f) for f in frames]
        if len(frames) < 2:
            raise ValueError("a tuple needs the reference frame and at least one source frame")
        out, world_T_cam, cam_T_world = self._prepare(frames, flip, native_depth_size)
        order = sort_sources_by_pose_penalty(cam_T_world[0], np.stack(world_T_cam[1:]))
        src = [out[1 + i] for i in order]
        src_data = {k: [s[k] for s in src] if k == "frame_id_string" else torch.stack([s[k] for s in src])
                    for k in src[0]}
        return out[0], src_data
