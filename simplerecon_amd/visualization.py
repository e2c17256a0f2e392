"""The reference's depth visualisation (utils/visualization_utils.py and the image log of its training step), API-compatible,
on the HIP kernels of csrc/sr_viz.hip.  The rules are stated in include/simplerecon_hip.h, section "visualisation".

    colormap_image(image_1hw, mask_1hw, ...)    the reference's function: fp32 [3,H,W] (or [B,3,H,W] from [B,1,H,W])
    colormap_u8(...)                            the same picture as 8-bit [B,H,W,3], ready for an image file
    normals_image / normals_u8, color_image / color_u8   0.5 * (1 + n) and the de-normalised input image
    quick_viz_export(...)                       test.py --dump_depth_visualization: four PNGs per frame
    training_images(cur_data, outputs)          the pictures the reference's training step logs

Every picture is one kernel launch (two more for an automatic value range) and stays on the device; nothing here
synchronises the host except quick_viz_export, which brings all pictures of a batch to the host in one copy and leaves
the PNG encoding to Pillow.  Inputs are fp32 device tensors; host tensors and other dtypes are refused (no CPU fallback).

Departures from the reference, all where it raises or is undefined: an empty selection gives a NaN range (and so table
entry 0 everywhere) where torch.min raises; 8-bit values are clamped to 0..255 where np.uint8 of an out-of-range float
is undefined; quick_viz_export without "frame_id_string" names files by the running index."""
import os

import torch

from . import _lib

MASK_NONE, MASK_U8, MASK_F32 = 0, 1, 2     # SR_VIZ_MASK_*
UNIT_NORMALS, UNIT_COLOR = 0, 1            # SR_VIZ_UNIT_*
MAX_PIXELS = 1 << 30                       # SR_VIZ_MAX_PIXELS
_FP32 = "the pictures are computed in fp32"

_TABLES = {}   # (name, flip, device) -> [256,3] fp32 device tensor


def colormap_table(colormap="turbo"):
    """[256,3] fp32 host tensor: matplotlib's `colormap` at linspace(0, 1, 256), as the reference builds it.  "turbo"
    ships with the package; any other name is built from matplotlib when asked for."""
    if colormap == "turbo":
        from ._turbo import TURBO
        return torch.tensor(TURBO, dtype=torch.float32)
    try:
        import matplotlib
    except ImportError as e:
        raise ImportError(f"colormap {colormap!r} is built from matplotlib, which is not installed (only 'turbo' ships "
                          "with simplerecon_amd; a [256,3] tensor is accepted in place of a name)") from e
    import numpy as np
    if not isinstance(colormap, str) or colormap not in matplotlib.colormaps:
        raise ValueError(f"colormap: matplotlib has no colour map named {colormap!r}")
    return torch.Tensor(matplotlib.colormaps[colormap](np.linspace(0, 1, 256))[:, :3])


def _table(colormap, flip, device):
    if isinstance(colormap, torch.Tensor):
        if colormap.dtype != torch.float32:
            raise TypeError(f"colormap must be float32, got {colormap.dtype}")
        if tuple(colormap.shape) != (256, 3):
            raise ValueError(f"colormap: expected a [256,3] table, got {tuple(colormap.shape)}")
        t = colormap.detach().to(device)
        return torch.flip(t, (0,)).contiguous() if flip else t.contiguous()
    key = (colormap, bool(flip), device)
    t = _TABLES.get(key)
    if t is None:
        t = colormap_table(colormap)
        t = _TABLES[key] = (torch.flip(t, (0,)) if flip else t).contiguous().to(device)
    return t


def _maps(name, t):
    """An fp32 device tensor [1,H,W] or [B,1,H,W] -> (contiguous tensor, B, H, W, batched)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t)}")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 ({_FP32}), got {t.dtype}")
    if t.dim() == 3 and t.shape[0] == 1:
        B, batched = 1, False
    elif t.dim() == 4 and t.shape[1] == 1:
        B, batched = t.shape[0], True
    else:
        raise ValueError(f"{name}: expected a [1,H,W] image or a [B,1,H,W] batch, got {tuple(t.shape)}")
    H, W = t.shape[-2:]
    if B < 1 or H * W < 1 or H * W > MAX_PIXELS:
        raise ValueError(f"{name}: empty or too large, got {tuple(t.shape)}")
    return _lib.device_f32(name, t, _FP32).detach(), B, H, W, batched


def _planes(name, t):
    """An fp32 device tensor [B,3,H,W] (or [3,H,W]) -> (contiguous tensor, B, H, W, batched)."""
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t)}")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 ({_FP32}), got {t.dtype}")
    if t.dim() not in (3, 4) or t.shape[-3] != 3 or t.numel() == 0 or t.shape[-2] * t.shape[-1] > MAX_PIXELS:
        raise ValueError(f"{name}: expected a [B,3,H,W] batch or a [3,H,W] image, got {tuple(t.shape)}")
    B = t.shape[0] if t.dim() == 4 else 1
    return _lib.device_f32(name, t, _FP32).detach(), B, t.shape[-2], t.shape[-1], t.dim() == 4


def _mask(name, t, like):
    """-> (contiguous mask, SR_VIZ_MASK_*): fp32 masks keep their values, bool / uint8 masks count as 1 / 0."""
    if t is None:
        return None, MASK_NONE
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor, got {type(t)}")
    if t.dtype not in (torch.float32, torch.bool, torch.uint8):
        raise TypeError(f"{name} must be a float32, bool or uint8 mask, got {t.dtype}")
    if t.numel() != like.numel():
        raise ValueError(f"{name} {tuple(t.shape)} does not cover the image {tuple(like.shape)}")
    if not t.is_cuda:
        raise _lib.HipLibraryError(f"{name} lives on {t.device}: the HIP path needs device tensors (no CPU fallback)")
    if t.device != like.device:
        raise ValueError(f"{name} is on {t.device}, the image on {like.device}")
    t = t.detach().contiguous()
    return (t, MASK_F32) if t.dtype == torch.float32 else (t.view(torch.uint8), MASK_U8)


def value_range(image, mask=None, pooled=False, out=None):
    """Minimum and maximum of the values of `image` ([B,1,H,W] or [1,H,W] fp32) selected by `mask` (non-zero): a device
    tensor [B,2], or [2] over the whole batch when pooled.  A selected NaN, or an empty selection, gives NaN for both.
    `out` (fp32, contiguous, of that shape) receives the result when given.  No host synchronisation."""
    image, B, H, W, _ = _maps("image", image)
    mask, kind = _mask("mask", mask, image)
    return _range(image, mask, kind, B, H * W, pooled, out)


def _range(image, mask, kind, B, n, pooled, out=None):
    dev = image.device
    if out is None:
        out = torch.empty((2,) if pooled else (B, 2), dtype=torch.float32, device=dev)
    nbytes = int(_lib.lib().sr_viz_range_workspace_bytes(B, n))
    if nbytes == 0:
        raise ValueError(f"value range: B={B} images of {n} pixels refused by the library")
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    _lib.call("sr_viz_range", dev, image, mask, kind, B, n, 1 if pooled else 0, out, ws, nbytes)
    return out


def _bound(name, v, B, device):
    """A given vmin / vmax -> (device tensor or None, its stride between images, host scalar)."""
    if isinstance(v, torch.Tensor):
        if v.dtype != torch.float32:
            raise TypeError(f"{name} must be float32, got {v.dtype}")
        if v.numel() not in (1, B):
            raise ValueError(f"{name}: expected one value or one per image ({B}), got {tuple(v.shape)}")
        if not v.is_cuda:
            raise _lib.HipLibraryError(f"{name} lives on {v.device}: pass a float or a device tensor (no CPU fallback)")
        if v.device != device:
            raise ValueError(f"{name} is on {v.device}, the image on {device}")
        v = v.detach().reshape(-1)   # (a column of a [B,2] range stays a view: the kernel takes its stride)
        return v, (0 if v.numel() == 1 else v.stride(0)), 0.0
    if isinstance(v, (int, float)):
        return None, 0, float(v)
    raise TypeError(f"{name} must be a float or a device tensor, got {type(v)}")


def _check_out(out, nbytes):
    if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous():
        raise TypeError("out must be a contiguous uint8 device tensor")
    if out.numel() != nbytes:
        raise ValueError(f"out holds {out.numel()} bytes, the picture {nbytes}")


def _colormap(image_1hw, mask_1hw, invalid_color, flip, vmin, vmax, colormap, want_f32, want_u8, out_u8=None):
    """-> (fp32 [B,3,H,W] or None, uint8 [B,H,W,3] or None, vmin, vmax as given / computed, batched).  out_u8: a
    contiguous uint8 device tensor of B*H*W*3 elements that receives the 8-bit picture in place of a new one."""
    image, B, H, W, batched = _maps("image_1hw", image_1hw)
    dev = image.device
    mask, kind = _mask("mask_1hw", mask_1hw, image)
    invalid = [float(c) for c in invalid_color]
    if len(invalid) != 3:
        raise ValueError(f"invalid_color: expected three components, got {invalid_color!r}")
    lut = _table(colormap, flip, dev)
    if vmin is None or vmax is None:
        auto = _range(image, mask, kind, B, H * W, False)   # (the reference's valid_vals.min() / .max())
        if vmin is None:
            vmin = auto[:, 0]
        if vmax is None:
            vmax = auto[:, 1]
    lo, lo_stride, lo_host = _bound("vmin", vmin, B, dev)
    hi, hi_stride, hi_host = _bound("vmax", vmax, B, dev)
    f32 = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev) if want_f32 else None
    u8 = None
    if out_u8 is not None:
        _check_out(out_u8, B * H * W * 3)
        u8 = out_u8
    elif want_u8:
        u8 = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    _lib.call("sr_viz_colormap", dev, image, mask, kind, B, H * W, lut, lo, lo_stride, hi, hi_stride, lo_host, hi_host,
              invalid[0], invalid[1], invalid[2], f32, u8)
    return f32, u8, vmin, vmax, batched


def _returned(v, batched, B, device):
    """vmin / vmax as the reference returns them: a 0-dim device tensor for one image, [B] for a batch."""
    if not isinstance(v, torch.Tensor):
        v = torch.full((), float(v), dtype=torch.float32, device=device)
    if not batched:
        return v.reshape(())
    return v.reshape(-1).expand(B) if v.numel() == 1 else v.reshape(B)


def colormap_image(image_1hw, mask_1hw=None, invalid_color=(0.0, 0, 0.0), flip=True, vmin=None, vmax=None,
                   return_vminvmax=False, colormap="turbo"):
    """The reference's colormap_image (utils/visualization_utils.py:12-72), bit for bit: `image_1hw` [1,H,W] fp32 ->
    fp32 [3,H,W] on its device; t = (x - vmin) / (vmax - vmin), table entry (int) clamp(t * 255, 0, 255), and with a
    mask rgb * mask + invalid_color * (1 - mask).  vmin / vmax default to the minimum / maximum of the values where the
    mask is non-zero (of all values without one); they may be floats or device tensors.  A [B,1,H,W] batch gives
    [B,3,H,W] with one range per image (a given range: one value, or B).  `colormap`: "turbo", any matplotlib name (needs
    matplotlib), or a [256,3] fp32 table.  With return_vminvmax the two come back as device tensors (0-dim; [B] for a
    batch).  NaN pixels get entry 0; a NaN or empty selection makes the automatic range NaN, and every pixel entry 0,
    where the reference raises on the empty selection.  No host synchronisation."""
    out, _, vmin, vmax, batched = _colormap(image_1hw, mask_1hw, invalid_color, flip, vmin, vmax, colormap, True, False)
    B = out.shape[0]
    if not batched:
        out = out[0]
    if return_vminvmax:
        return out, _returned(vmin, batched, B, out.device), _returned(vmax, batched, B, out.device)
    return out


def colormap_u8(image_1hw, mask_1hw=None, invalid_color=(0.0, 0, 0.0), flip=True, vmin=None, vmax=None,
                return_vminvmax=False, colormap="turbo", out=None):
    """colormap_image as 8-bit pixels, uint8 [B,H,W,3] ([H,W,3] for one [1,H,W] image): np.uint8(rgb * 255) of the fp32
    picture, as the reference writes its PNGs.  `out`: a contiguous uint8 device tensor of that many elements to write
    into; it is returned as it is."""
    _, pic, vmin, vmax, batched = _colormap(image_1hw, mask_1hw, invalid_color, flip, vmin, vmax, colormap, False, True,
                                            out)
    B = image_1hw.shape[0] if batched else 1
    if out is None and not batched:
        pic = pic[0]
    if return_vminvmax:
        return pic, _returned(vmin, batched, B, pic.device), _returned(vmax, batched, B, pic.device)
    return pic


def _unit(name, t, mode, want_f32, out_u8=None):
    x, B, H, W, batched = _planes(name, t)
    dev = x.device
    f32 = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev) if want_f32 else None
    if out_u8 is not None:
        _check_out(out_u8, B * H * W * 3)
    elif not want_f32:
        out_u8 = torch.empty((B, H, W, 3) if batched else (H, W, 3), dtype=torch.uint8, device=dev)
    _lib.call("sr_viz_unit", dev, x, B, H * W, mode, f32, out_u8)
    if want_f32:
        return f32 if batched else f32[0]
    return out_u8


def normals_image(normals_b3hw):
    """nan_to_num(0.5 * (1 + n)) of [B,3,H,W] (or [3,H,W]) fp32 normals: the fp32 picture of the reference's training
    log and video columns."""
    return _unit("normals_b3hw", normals_b3hw, UNIT_NORMALS, True)


def normals_u8(normals_b3hw, out=None):
    """normals_image as 8-bit pixels, uint8 [B,H,W,3]."""
    return _unit("normals_b3hw", normals_b3hw, UNIT_NORMALS, False, out)


def color_image(image_b3hw):
    """The reference's reverse_imagenet_normalize (utils/generic_utils.py:153-159) of an ImageNet-normalised image:
    (x - mean_c) / std_c with its constants, fp32 [B,3,H,W]."""
    return _unit("image_b3hw", image_b3hw, UNIT_COLOR, True)


def color_u8(image_b3hw, out=None):
    """color_image as 8-bit pixels, uint8 [B,H,W,3]; values outside [0, 1] are clamped."""
    return _unit("image_b3hw", image_b3hw, UNIT_COLOR, False, out)


def quick_viz_pictures(outputs, cur_data, valid_mask_b):
    """The device part of quick_viz_export: one flat uint8 device buffer holding, in this order, (B + 1) fp32 (min, max)
    pairs as raw bytes -- the range of each sample's valid ground truth, then the batch's colour range -- and the 8-bit
    pictures [B,H,W,3] of the ground truth, [B,h,w,3] of the lowest-cost depth, [B,h,w,3] of the prediction and
    [B,Hc,Wc,3] of the colour image; plus the four picture shapes.  No host synchronisation."""
    gt = cur_data["full_res_depth_b1hw"]
    pred = outputs["depth_pred_s0_b1hw"]
    lowest = outputs["lowest_cost_bhw"]
    color = cur_data["high_res_color_b3hw"] if "high_res_color_b3hw" in cur_data else cur_data["image_b3hw"]
    gt, B, H, W, _ = _maps("full_res_depth_b1hw", gt if gt.dim() == 4 else gt.unsqueeze(1))
    if lowest.dim() == 3:
        lowest = lowest.unsqueeze(1)
    if pred.shape[0] != B or lowest.shape[0] != B or color.shape[0] != B:
        raise ValueError(f"batch sizes differ: ground truth {B}, prediction {pred.shape[0]}, lowest cost "
                         f"{lowest.shape[0]}, colour {color.shape[0]}")
    valid, kind = _mask("valid_mask_b", valid_mask_b, gt)
    dev = gt.device
    shapes = [(B, H, W, 3), (B,) + tuple(lowest.shape[-2:]) + (3,), (B,) + tuple(pred.shape[-2:]) + (3,),
              (B,) + tuple(color.shape[-2:]) + (3,)]
    head = (B + 1) * 8
    sizes = [s[0] * s[1] * s[2] * s[3] for s in shapes]
    buf = torch.empty(head + sum(sizes), dtype=torch.uint8, device=dev)
    ranges = buf[:head].view(torch.float32).view(B + 1, 2)
    _range(gt, valid, kind, B, H * W, False, ranges[:B])
    batch = _range(gt, valid, kind, B, H * W, True, ranges[B])
    # nothing valid (a NaN range here) or a constant ground truth: 0..5 (visualization_utils.py:93-102)
    default = torch.isnan(batch[0]) | (batch[0] == batch[1])
    batch.copy_(torch.where(default, torch.stack([torch.zeros_like(batch[0]), torch.full_like(batch[1], 5.0)]), batch))
    slots, start = [], head
    for size in sizes:
        slots.append(buf[start:start + size])
        start += size
    for image, slot in zip((gt, lowest, pred), slots):
        _colormap(image, None, (0.0, 0.0, 0.0), True, batch[0], batch[1], "turbo", False, True, slot)
    color_u8(color, slots[3])
    return buf, shapes


def quick_viz_export(output_path, outputs, cur_data, batch_ind, valid_mask_b, batch_size):
    """The reference's quick_viz_export (utils/visualization_utils.py:84-167): for every sample of the batch writes
    {frame_id}_gt_depth.png, {frame_id}_lowest_cost_pred.png, {frame_id}_pred_depth.png and {frame_id}_color.png into
    `output_path`.  The three depth pictures share the batch's colour range: minimum and maximum of
    full_res_depth_b1hw over valid_mask_b, or 0..5 when nothing is valid or the two are equal.  A sample without a valid
    value, or with a constant valid ground truth, gets no _gt_depth.png.  The colour picture is the de-normalised
    high_res_color_b3hw (image_b3hw when the batch has none, where the reference raises KeyError).

    frame_id is cur_data["frame_id_string"][i]; without that key the reference fails (it formats a str with `:6d`), here
    it is the running index batch_ind * batch_size + i as six zero-padded digits.

    All pictures are made on the device and reach the host in one copy; Pillow encodes the PNGs.  Returns the list of
    file names written."""
    from PIL import Image
    buf, shapes = quick_viz_pictures(outputs, cur_data, valid_mask_b)
    host = buf.cpu()   # the one device-to-host copy
    B = shapes[0][0]
    ranges = host[:(B + 1) * 8].view(torch.float32).view(B + 1, 2).numpy()
    pictures, start = [], (B + 1) * 8
    for s in shapes:
        size = s[0] * s[1] * s[2] * s[3]
        pictures.append(host[start:start + size].view(s).numpy())
        start += size
    written = []
    for i in range(B):
        if "frame_id_string" in cur_data:
            frame_id = cur_data["frame_id_string"][i]
        else:
            frame_id = f"{batch_ind * batch_size + i:06d}"
        lo, hi = ranges[i]
        names = [None if (lo != lo or lo == hi) else "gt_depth", "lowest_cost_pred", "pred_depth", "color"]
        for name, pics in zip(names, pictures):
            if name is not None:
                written.append(f"{frame_id}_{name}.png")
                Image.fromarray(pics[i]).save(os.path.join(output_path, written[-1]))
    return written


def training_images(cur_data, outputs, count=4):
    """The pictures the reference's training step logs every log_every_n_steps (depth_model.py:542-562), as a dict of
    fp32 [3,H,W] device tensors: image/i (de-normalised image_b3hw), depth_gt/i (depth_b1hw colour-mapped under
    mask_b1hw, automatic range), depth_pred/i, depth_pred_lr/i (depth_pred_s3_b1hw) and cv_min/i (lowest_cost_bhw) in the
    ground truth's range, normals_gt/i and normals_pred/i (cur_data["normals_b3hw"] and outputs["normals_pred_b3hw"] as
    DepthModel.step leaves them; NaN normals become 0), for i < min(count, B).  No host synchronisation."""
    depth_gt = cur_data["depth_b1hw"]
    n = min(int(count), depth_gt.shape[0])
    with torch.no_grad():
        gt, vmin, vmax = colormap_image(depth_gt[:n], cur_data["mask_b1hw"][:n], return_vminvmax=True)
        pred = colormap_image(outputs["depth_pred_s0_b1hw"][:n], vmin=vmin, vmax=vmax)
        pred_lr = colormap_image(outputs["depth_pred_s3_b1hw"][:n], vmin=vmin, vmax=vmax)
        cv_min = colormap_image(outputs["lowest_cost_bhw"][:n].unsqueeze(1), vmin=vmin, vmax=vmax)
        image = color_image(cur_data["image_b3hw"][:n])
        normals_gt = normals_image(cur_data["normals_b3hw"][:n])
        normals_pred = normals_image(outputs["normals_pred_b3hw"][:n])
    out = {}
    for i in range(n):
        out[f"image/{i}"] = image[i]
        out[f"depth_gt/{i}"] = gt[i]
        out[f"depth_pred/{i}"] = pred[i]
        out[f"depth_pred_lr/{i}"] = pred_lr[i]
        out[f"normals_gt/{i}"] = normals_gt[i]
        out[f"normals_pred/{i}"] = normals_pred[i]
        out[f"cv_min/{i}"] = cv_min[i]
    return out
