"""Writes tests/golden/viz_cm_<case>.npz and tests/golden/viz_quick_<batch>.npz: what the reference's OWN
utils/visualization_utils.py (colormap_image, quick_viz_export) computes on the CPU.  Needs a checkout of the reference
(pass its root), matplotlib and Pillow.

    python tests/golden/make_viz_golden.py /path/to/simplerecon

visualization_utils.py imports moviepy.editor (video export, never reached here) and, through utils/generic_utils.py,
kornia and torchvision: oracle/refshim.py's stubs serve those, an empty moviepy.editor is added here, and
torchvision.transforms.functional.normalize -- which reverse_imagenet_normalize calls -- is given its published definition,
(tensor - mean[:, None, None]) / std[:, None, None].  The _color.png pictures rest on that definition, not on
torchvision's code; everything else is the reference's code alone.

viz_cm_<case>.npz: image [1,H,W] (or [B,1,H,W]: B separate calls), optional mask, invalid_color, flip, colormap, optional
given vmin / vmax, and the results out [3,H,W] (or [B,3,H,W]), vmin_out, vmax_out.
viz_quick_<batch>.npz: gt [B,1,H,W], valid [B,1,H,W], lowest [B,h,w], pred [B,1,h,w], color [B,3,H,W], frame_ids, names
(the files written, sorted) and png_<file name>: each file decoded."""
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
F32 = np.float32


def _ulps(x, k):
    x = F32(x)
    for _ in range(abs(k)):
        x = np.nextafter(x, F32(np.inf if k > 0 else -np.inf), dtype=F32)
    return x


def _bin_edges(vmin, vmax):
    """Inputs whose t * 255 lands on, and a few ulps either side of, the integers 0, 1, 2, 127, 128, 254 and 255 --
    254.9999..., 255 and just below 0 among them."""
    xs = []
    for k in (0, 1, 2, 127, 128, 254, 255):
        x0 = F32(F32(vmin) + F32(F32(vmax) - F32(vmin)) * F32(k) / F32(255))
        xs += [_ulps(x0, j) for j in range(-3, 4)]
    xs += [F32(vmin), F32(vmax), _ulps(vmin, -1), _ulps(vmax, -1), _ulps(vmax, 1)]
    return np.array(xs, F32)


def colormap_cases():
    rng = np.random.default_rng(512)
    out = {}
    depth = lambda *s: rng.uniform(0.3, 6.0, size=s).astype(F32)
    out["plain"] = dict(image=depth(1, 7, 13))
    img = depth(1, 9, 14)
    out["mask01"] = dict(image=img, mask=(rng.uniform(size=img.shape) < 0.6).astype(F32), invalid_color=(0.2, 0.4, 0.6))
    img = depth(1, 9, 14)
    out["mask_fraction"] = dict(image=img, mask=rng.choice(np.array([0.0, 0.5, 1.0], F32), size=img.shape),
                                invalid_color=(0.9, 0.1, 0.3))
    out["noflip"] = dict(image=depth(1, 7, 13), flip=False)
    out["viridis"] = dict(image=depth(1, 7, 13), colormap="viridis")
    out["given_range"] = dict(image=depth(1, 8, 12), vmin=1.5, vmax=4.0)     # values below vmin and above vmax
    e1, e2 = _bin_edges(0.5, 4.5), _bin_edges(0.0, 255.0)
    out["bin_edges"] = dict(image=e1.reshape(1, 1, -1), vmin=0.5, vmax=4.5)
    out["bin_edges_255"] = dict(image=e2.reshape(1, 1, -1), vmin=0.0, vmax=255.0)
    img = depth(1, 5, 9)
    img[0, 0, :3] = [np.nan, np.inf, -np.inf]
    img[0, 3, 4] = np.nan
    out["nonfinite"] = dict(image=img, vmin=0.5, vmax=5.0)
    img = depth(1, 4, 6)
    img[0, 1, :3] = 2.0
    out["equal_range"] = dict(image=img, vmin=2.0, vmax=2.0)
    img = depth(1, 6, 7)
    img[0, 2, 2] = np.nan
    m = np.ones_like(img)
    m[0, 0, :] = 0
    out["nan_valid"] = dict(image=img, mask=m, invalid_color=(0.5, 0.5, 0.5))
    out["multi_block"] = dict(image=depth(3, 1, 97, 131))
    bits = rng.integers(0, 1 << 23, size=(1, 6, 11), dtype=np.uint32)
    bits |= (rng.integers(0, 2, size=bits.shape, dtype=np.uint32) << np.uint32(31))
    out["denormal"] = dict(image=bits.view(F32))
    return out


def run_colormap(vu, case):
    img = torch.from_numpy(case["image"])
    images = [img] if img.dim() == 3 else list(img)
    kw = {k: case[k] for k in ("invalid_color", "flip", "vmin", "vmax", "colormap") if k in case}
    outs, los, his = [], [], []
    for i, im in enumerate(images):
        mask = None
        if "mask" in case:
            mask = torch.from_numpy(case["mask"] if img.dim() == 3 else case["mask"][i])
        o, lo, hi = vu.colormap_image(im, mask, return_vminvmax=True, **kw)
        outs.append(o.numpy().astype(F32))
        los.append(np.asarray(float(lo), np.float64).astype(F32))
        his.append(np.asarray(float(hi), np.float64).astype(F32))
    if img.dim() == 3:
        return outs[0], los[0], his[0]
    return np.stack(outs), np.stack(los), np.stack(his)


def quick_cases():
    rng = np.random.default_rng(640)
    B, H, W, h, w = 3, 12, 16, 6, 8
    std = np.array([4.36681223, 4.46428571, 4.44444444], F32)[None, :, None, None]
    mean = np.array([-2.11790393, -2.03571429, -1.80444444], F32)[None, :, None, None]

    def batch():
        gt = rng.uniform(0.6, 5.0, size=(B, 1, H, W)).astype(F32)
        gt[:, :, ::5, ::3] = 0.0          # holes
        gt[:, :, 1, 1] = np.nan
        return dict(gt=gt, lowest=rng.uniform(0.3, 6.0, size=(B, h, w)).astype(F32),
                    pred=rng.uniform(0.3, 6.0, size=(B, 1, h, w)).astype(F32),
                    color=(rng.uniform(0.01, 0.99, size=(B, 3, H, W)).astype(F32) * std + mean).astype(F32))
    out = {"ordinary": batch()}
    c = batch()
    c["gt"][1] = 0.25
    c["gt"][1, 0, 2, :4] = np.nan
    out["sample_invalid"] = c
    c = batch()
    c["gt"][2] = 2.0
    c["gt"][2, 0, ::4] = 0.0
    out["sample_constant"] = c
    c = batch()
    c["gt"][:] = rng.uniform(0.0, 0.5, size=c["gt"].shape).astype(F32)
    out["nothing_valid"] = c
    for k, (name, c) in enumerate(out.items()):
        c["frame_ids"] = [f"{100 * k + 7 * i:06d}" for i in range(B)]
    return out


def run_quick(vu, case):
    from PIL import Image
    gt = torch.from_numpy(case["gt"])
    valid = gt > 0.5
    cur = {"full_res_depth_b1hw": gt, "high_res_color_b3hw": torch.from_numpy(case["color"]),
           "frame_id_string": list(case["frame_ids"])}
    outputs = {"depth_pred_s0_b1hw": torch.from_numpy(case["pred"]), "lowest_cost_bhw": torch.from_numpy(case["lowest"])}
    res = {"valid": valid.numpy()}
    with tempfile.TemporaryDirectory() as d:
        vu.quick_viz_export(d, outputs, cur, 0, valid, gt.shape[0])
        names = sorted(os.listdir(d))
        for n in names:
            res[f"png_{n}"] = np.array(Image.open(os.path.join(d, n)))
    res["names"] = np.array(names)
    return res


def import_reference(ref_root):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import refshim
    refshim.install_stubs()
    for name in ("moviepy", "moviepy.editor"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["moviepy"].editor = sys.modules["moviepy.editor"]

    def normalize(tensor, mean, std):
        mean = torch.as_tensor(mean, dtype=tensor.dtype)
        std = torch.as_tensor(std, dtype=tensor.dtype)
        return (tensor - mean[:, None, None]) / std[:, None, None]
    sys.modules["torchvision.transforms.functional"].normalize = normalize
    sys.path.insert(0, ref_root)
    return importlib.import_module("utils.visualization_utils")


def main(ref_root):
    vu = import_reference(ref_root)
    for name, case in colormap_cases().items():
        out, lo, hi = run_colormap(vu, case)
        arrays = {k: np.asarray(v) for k, v in case.items()}
        arrays.update(out=out, vmin_out=lo, vmax_out=hi)
        path = os.path.join(HERE, f"viz_cm_{name}.npz")
        np.savez_compressed(path, **arrays)
        print(f"wrote {path} ({os.path.getsize(path)} bytes)")
    for name, case in quick_cases().items():
        arrays = {k: np.asarray(v) for k, v in case.items()}
        arrays.update(run_quick(vu, case))
        path = os.path.join(HERE, f"viz_quick_{name}.npz")
        np.savez_compressed(path, **arrays)
        print(f"wrote {path} ({os.path.getsize(path)} bytes)  files: {len(arrays['names'])}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
