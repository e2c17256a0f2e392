"""numpy restatement of the frame-preparation kernels (csrc/sr_frames.hip), driven by the same host tables
(simplerecon_amd.frames.resample_tables / nearest_table): what the GPU results and Pillow's are compared with."""
import numpy as np
import torch

from simplerecon_amd import frames


def _wrap32(a):
    """int64 sums folded into the 32-bit two's-complement range, as the kernels' integer arithmetic wraps."""
    return ((a + (1 << 31)) % (1 << 32)) - (1 << 31)


def resize_pass(img_bhwc, axis, out_size, resample):
    """One pass along axis 1 (rows: the vertical pass) or 2 (columns: the horizontal pass) of uint8 [B,h,w,C]."""
    first, count, weights = frames.resample_tables(img_bhwc.shape[axis], out_size, resample)
    src = np.moveaxis(img_bhwc, axis, 0).astype(np.int64)
    out = np.empty((out_size,) + src.shape[1:], dtype=np.uint8)
    for i in range(out_size):
        acc = np.full(src.shape[1:], 1 << (frames.PRECISION_BITS - 1), dtype=np.int64)
        for k in range(count[i]):
            acc = _wrap32(acc + src[first[i] + k] * int(weights[i, k]))
        out[i] = np.clip(acc >> frames.PRECISION_BITS, 0, 255)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def resize_u8(img_bhwc, height, width, resample="bilinear"):
    """Horizontal pass, rounded to uint8, then vertical pass: uint8 [B,H,W,C]."""
    return resize_pass(resize_pass(img_bhwc, 2, width, resample), 1, height, resample)


def prepare_color(img_bhw3, height, width, resample="bilinear", flip=False):
    small = resize_u8(img_bhw3, height, width, resample)
    if flip:
        small = small[:, :, ::-1]
    lut = frames.normalise_table().numpy()
    return np.stack([lut[c][small[..., c]] for c in range(3)], axis=1)


def prepare_depth(depth_bhw, height=None, width=None, scale=1e-3, min_valid=1e-3, max_valid=10.0, flip=False):
    h, w = depth_bhw.shape[1:]
    H, W = (h, w) if height is None else (height, width)
    ys, xs = frames.nearest_table(h, H), frames.nearest_table(w, W)
    d = depth_bhw[:, ys][:, :, xs].astype(np.float32) * np.float32(scale)
    if flip:
        d = d[:, :, ::-1]
    ok = (d > np.float32(min_valid)) & (d < np.float32(max_valid))
    d = np.where(ok, d, np.float32(np.nan)).astype(np.float32)
    return d[:, None], ok.astype(np.float32)[:, None], ok[:, None]
