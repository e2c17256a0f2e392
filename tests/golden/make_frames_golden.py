"""Writes tests/golden/frames_{color,depth,tuple}.npz: inputs of the frame-preparation tests (tests/frames_cases.py)
and what the reference's loader makes of them, computed here with Pillow and torch's CPU kernels.

    python tests/golden/make_frames_golden.py

Colour: Image.resize, then torch.from_numpy(...).permute(2, 0, 1).float().div(255) (to_tensor), the optional flip,
then sub_(mean).div_(std) (TF.normalize).  Depth: a NEAREST resize of the 16-bit image, .float() * 1e-3, the two
comparisons and the NaN fill (scannet_dataset.py:499-513).  Intrinsics and poses: the operations of
scannet_dataset.py:450-470 and generic_mvs_dataset.py:508-512, 643-659 restated.  Every file records the Pillow
version that wrote it.  One-channel images go through mode "L", three through "RGB", four through "CMYK" (four
independent channels; Pillow premultiplies "RGBA")."""
import os
import sys

import numpy as np
import PIL
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import frames_cases as fc  # noqa: E402

MODES = {1: "L", 3: "RGB", 4: "CMYK"}
RESAMPLE = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC, "lanczos": Image.LANCZOS, "box": Image.BOX,
            "hamming": Image.HAMMING}
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def pil_resize(img_hwc, H, W, resample):
    C = img_hwc.shape[2]
    pil = Image.fromarray(img_hwc[..., 0] if C == 1 else img_hwc, MODES[C])
    if pil.size != (W, H):
        pil = pil.resize((W, H), resample=RESAMPLE[resample])
    return np.asarray(pil).reshape(H, W, C).copy()


def normalise(u8_hw3, flip):
    image = torch.from_numpy(u8_hw3).permute(2, 0, 1).contiguous().float().div(255)
    if flip:
        image = torch.flip(image, (-1,))
    mean = torch.as_tensor(MEAN, dtype=image.dtype).view(-1, 1, 1)
    std = torch.as_tensor(STD, dtype=image.dtype).view(-1, 1, 1)
    return image.clone().sub_(mean).div_(std).numpy()


def depth_and_masks(depth_hw, H, W, flip, min_valid=1e-3, max_valid=10.0):
    pil = Image.fromarray(depth_hw)
    assert pil.mode == "I;16"
    if H is not None and pil.size != (W, H):
        pil = pil.resize((W, H), resample=Image.NEAREST)
    depth = torch.from_numpy(np.asarray(pil).astype(np.int32))[None].float() * 1e-3
    mask_b = (depth > min_valid) & (depth < max_valid)
    mask = mask_b.float()
    depth[~mask_b] = torch.tensor(np.nan)
    if flip:
        depth, mask, mask_b = (torch.flip(t, (-1,)) for t in (depth, mask, mask_b))
    return depth.numpy(), mask.numpy(), mask_b.numpy()


def intrinsics(K_44, native_w, native_h, depth_w, depth_h, flip, full):
    out = {}
    K = torch.tensor(K_44.astype(np.float32))
    if flip:
        K[0, 2] = float(native_w) - K[0, 2]
    if full:
        out["K_full_depth_b44"] = K.clone().numpy()
        out["invK_full_depth_b44"] = np.linalg.inv(K)
    K[0] *= depth_w / float(native_w)
    K[1] *= depth_h / float(native_h)
    for i in range(5):
        K_scaled = K.clone()
        K_scaled[:2] /= 2 ** i
        out[f"K_s{i}_b44"] = K_scaled.numpy()
        out[f"invK_s{i}_b44"] = np.linalg.inv(K_scaled)
    return out


def pose_pair(world_T_cam, flip):
    world_T_cam = world_T_cam.astype(np.float32)
    if flip:
        T = np.eye(4).astype(world_T_cam.dtype)
        T[0, 0] = -1.0
        world_T_cam = world_T_cam @ T
    return world_T_cam, np.linalg.inv(world_T_cam)


def source_order(cur_cam_T_world, src_world_T_cam):
    pose = torch.tensor(cur_cam_T_world).unsqueeze(0) @ torch.tensor(src_world_T_cam)
    R_trace = pose[:, :3, :3].diagonal(offset=0, dim1=-1, dim2=-2).sum(-1)
    R_measure = torch.sqrt(2 * (1 - torch.minimum(torch.ones_like(R_trace) * 3.0, R_trace) / 3))
    t_measure = torch.norm(pose[:, :3, 3], dim=1)
    return torch.argsort(torch.sqrt(t_measure ** 2 + R_measure ** 2)).numpy()


def make_color():
    out = {"pillow_version": np.array(PIL.__version__)}
    for name, (B, h, w, C, H, W) in fc.COLOR_CASES.items():
        img = fc.color_input(name)
        out[f"in_{name}"] = img
        small = np.stack([pil_resize(img[b], H, W, "bilinear") for b in range(B)])
        out[f"u8_{name}"] = small
        if C == 3:
            out[f"f32_{name}"] = np.stack([normalise(s, False) for s in small])
        if name in fc.FLIP_CASES:
            out[f"f32flip_{name}"] = np.stack([normalise(s, True) for s in small])
    for filt in fc.OTHER_FILTERS:
        for name in fc.FILTER_CASES:
            B, h, w, C, H, W = fc.COLOR_CASES[name]
            out[f"u8_{filt}_{name}"] = np.stack([pil_resize(out[f"in_{name}"][b], H, W, filt) for b in range(B)])
    return out


def make_depth():
    out = {"pillow_version": np.array(PIL.__version__)}
    for name, (h, w, H, W) in fc.DEPTH_CASES.items():
        d = fc.depth_input(name)
        out[f"in_{name}"] = d
        for flip in (False, True):
            res = [depth_and_masks(d[b], H, W, flip) for b in range(d.shape[0])]
            tag = "flip_" if flip else ""
            out[f"depth_{tag}{name}"] = np.stack([r[0] for r in res])
            out[f"mask_{tag}{name}"] = np.stack([r[1] for r in res])
            out[f"mask_b_{tag}{name}"] = np.stack([r[2] for r in res])
    return out


def _rot(axis, angle):
    x, y, z = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


def make_tuple():
    """A reference frame and three sources, 97 x 131 colour and 48 x 64 depth, through get_frame / __getitem__ with the
    options of frames_cases.TUPLE; flipped and not (the flipped colour images are not stored: normalisation is
    element-wise, so they are the plain ones mirrored; prepare_color's flip has fixtures of its own in
    frames_color.npz).  The sources are given in an order the pose penalty changes."""
    cfg = fc.TUPLE
    rng = np.random.default_rng(7)
    n, ch, cw, dh, dw = 4, 97, 131, 48, 64
    colors = rng.integers(0, 256, (n, ch, cw, 3), dtype=np.uint8)
    colors[:, :20, :30] = 0
    colors[:, :20, 30:60] = 255
    depths = rng.integers(0, 11000, (n, dh, dw)).astype(np.uint16)
    depths[:, 0, : len(fc.DEPTH_SPECIALS)] = fc.DEPTH_SPECIALS
    base = np.eye(4)
    base[:3, :3] = _rot((0.3, 1.0, -0.2), 0.7)
    base[:3, 3] = (0.4, -0.3, 1.1)
    poses = [base]
    for angle, t in ((0.30, (0.5, 0.1, 0.0)), (0.05, (0.1, 0.0, 0.02)), (0.15, (-0.25, 0.05, 0.1))):
        d = np.eye(4)
        d[:3, :3] = _rot((0.2, 1.0, 0.1), angle)
        d[:3, 3] = t
        poses.append(base @ d)
    poses = np.stack(poses).astype(np.float32)
    K = np.eye(4, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 57.7, 57.9, 31.3, 24.1
    out = {"pillow_version": np.array(PIL.__version__), "colors": colors, "depths": depths, "world_T_cam": poses, "K": K}
    for flip in (False, True):
        frames = []
        for i in range(n):
            f = {}
            f["world_T_cam_b44"], f["cam_T_world_b44"] = pose_pair(poses[i], flip)
            f["image_b3hw"] = normalise(pil_resize(colors[i], cfg["image_height"], cfg["image_width"], "bilinear"), flip)
            f.update(intrinsics(K, dw, dh, cfg["depth_width"], cfg["depth_height"], flip, True))
            f["depth_b1hw"], f["mask_b1hw"], f["mask_b_b1hw"] = depth_and_masks(depths[i], cfg["depth_height"],
                                                                                cfg["depth_width"], flip)
            f["high_res_color_b3hw"] = normalise(pil_resize(colors[i], cfg["high_res_image_height"],
                                                            cfg["high_res_image_width"], "bilinear"), flip)
            f["full_res_depth_b1hw"], f["full_res_mask_b1hw"], f["full_res_mask_b_b1hw"] = depth_and_masks(
                depths[i], None, None, flip)
            frames.append(f)
        order = source_order(frames[0]["cam_T_world_b44"], np.stack([f["world_T_cam_b44"] for f in frames[1:]]))
        tag = "flip" if flip else "plain"
        out[f"{tag}_order"] = order.astype(np.int64)
        for k, v in frames[0].items():
            if flip and k in ("image_b3hw", "high_res_color_b3hw"):
                continue   # (the mirror image of the plain ones, element for element: left out to keep the file small)
            out[f"{tag}_cur_{k}"] = v
            out[f"{tag}_src_{k}"] = np.stack([frames[1 + i][k] for i in order])
    return out


if __name__ == "__main__":
    for kind, make in (("color", make_color), ("depth", make_depth), ("tuple", make_tuple)):
        path = os.path.join(HERE, f"frames_{kind}.npz")
        np.savez_compressed(path, **make())
        print(path, os.path.getsize(path))
