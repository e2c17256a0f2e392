"""Writes tests/golden/loss_<case>.npz: the inputs of tests/loss_cases.py and what the reference's OWN code computes
from them on the CPU -- its losses.py classes, its TorchScript NormalGenerator, and DepthModel.compute_losses called
unbound on a namespace holding the reference's loss modules.  Needs a checkout of the reference; pass its root.

kornia is not installed here: this process installs a scriptable `kornia.filters` written to the definitions of
include/simplerecon_hip.h ("training losses"; kornia 0.6.7's blur_pool2d, spatial_gradient, gaussian_blur2d), plus
empty torchvision / pytorch_lightning / timm / moviepy / antialiased_cnns stubs so that the reference imports.

    python tests/golden/make_loss_golden.py /path/to/simplerecon
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import loss_cases  # noqa: E402

KORNIA_FILTERS = '''
from typing import Tuple
import torch
import torch.nn.functional as F


def blur_pool2d(input: torch.Tensor, kernel_size: int, stride: int = 2) -> torch.Tensor:
    k = torch.tensor([1.0, 2.0, 1.0], dtype=input.dtype, device=input.device)
    k2 = (k[:, None] * k[None, :]) / 16.0
    k2 = k2.view(1, 1, 3, 3).repeat(input.shape[1], 1, 1, 1)
    return F.conv2d(input, k2, padding=1, stride=stride, groups=input.shape[1])


def spatial_gradient(input: torch.Tensor) -> torch.Tensor:
    sx = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]], dtype=input.dtype,
                      device=input.device) / 8.0
    b, c, h, w = input.shape
    k = torch.stack([sx, sx.t()]).unsqueeze(1).repeat(c, 1, 1, 1)
    xp = F.pad(input, [1, 1, 1, 1], mode="replicate")
    return F.conv2d(xp, k, groups=c).view(b, c, 2, h, w)


def gaussian_blur2d(input: torch.Tensor, kernel_size: Tuple[int, int], sigma: Tuple[float, float]) -> torch.Tensor:
    t = torch.arange(5, dtype=input.dtype, device=input.device) - 2.0
    g = torch.exp(-(t * t) / (2.0 * sigma[0] * sigma[0]))
    g = g / g.sum()
    k = (g[:, None] * g[None, :]).view(1, 1, 5, 5).repeat(input.shape[1], 1, 1, 1)
    return F.conv2d(F.pad(input, [2, 2, 2, 2], mode="reflect"), k, groups=input.shape[1])
'''


def install_shims():
    d = tempfile.mkdtemp(prefix="kornia_shim_")
    os.makedirs(os.path.join(d, "kornia"))
    with open(os.path.join(d, "kornia", "__init__.py"), "w") as f:
        f.write("from . import filters\n")
    with open(os.path.join(d, "kornia", "filters.py"), "w") as f:
        f.write(KORNIA_FILTERS)
    sys.path.insert(0, d)

    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    tv = mod("torchvision")
    tv.transforms = mod("torchvision.transforms")
    tv.transforms.functional = mod("torchvision.transforms.functional")
    tv.models = mod("torchvision.models")
    tv.ops = mod("torchvision.ops", FeaturePyramidNetwork=object)
    mod("timm")
    mod("antialiased_cnns")
    mod("pytorch_lightning", LightningModule=torch.nn.Module)
    mod("moviepy")
    mod("moviepy.editor")


def main(ref_root):
    sys.path.insert(0, ref_root)
    install_shims()
    import losses as rl
    from experiment_modules.depth_model import DepthModel
    from utils.geometry_utils import NormalGenerator
    for name in loss_cases.CASES:
        c = loss_cases.case(name)
        t = {k: torch.from_numpy(v) for k, v in c.items()}
        B, _, h, w = t["depth_b1hw"].shape
        ns = types.SimpleNamespace(si_loss=rl.ScaleInvariantLoss(), grad_loss=rl.MSGradientLoss(),
                                   abs_loss=torch.nn.L1Loss(), normals_loss=rl.NormalsLoss(),
                                   mv_depth_loss=rl.MVDepthLoss(h, w))
        ns.ms_loss_fn = ns.abs_loss
        gen = NormalGenerator(h, w)
        scales = [i for i in range(4) if f"log_depth_pred_s{i}_b1hw" in t]
        pred = t["depth_pred_s0_b1hw"].clone().requires_grad_(True)
        logs = {i: t[f"log_depth_pred_s{i}_b1hw"].clone().requires_grad_(True) for i in scales}
        cur = {"depth_b1hw": t["depth_b1hw"], "mask_b_b1hw": t["mask_b_b1hw"], "mask_b1hw": t["mask_b_b1hw"].float(),
               "invK_s0_b44": t["invK_s0_b44"], "world_T_cam_b44": t["world_T_cam_b44"]}
        src = {"depth_b1hw": t["src_depth_bk1hw"], "K_s0_b44": t["src_K_s0_bk44"],
               "cam_T_world_b44": t["src_cam_T_world_bk44"]}
        cur["normals_b3hw"] = gen(t["depth_b1hw"], t["invK_s0_b44"])
        outputs = {"depth_pred_s0_b1hw": pred, "normals_pred_b3hw": gen(pred, t["invK_s0_b44"])}
        outputs.update({f"log_depth_pred_s{i}_b1hw": v for i, v in logs.items()})
        terms = DepthModel.compute_losses(ns, cur, src, outputs)
        out = dict(c)
        out["normals_gt"] = cur["normals_b3hw"].detach().numpy()
        out["normals_pred"] = outputs["normals_pred_b3hw"].detach().numpy()
        leaves = [pred] + [logs[i] for i in scales]
        names = ["depth_pred_s0_b1hw"] + [f"log_depth_pred_s{i}_b1hw" for i in scales]
        for key, v in terms.items():
            out[f"term/{key}"] = np.float32(v.detach())
            if not v.requires_grad:
                continue
            gs = torch.autograd.grad(v, leaves, retain_graph=True, allow_unused=True)
            for n, g in zip(names, gs):
                out[f"grad/{key}/{n}"] = (torch.zeros_like(leaves[names.index(n)]) if g is None else g).numpy()
        path = os.path.join(HERE, f"loss_{name}.npz")
        np.savez_compressed(path, **out)
        print(f"{path}: " + ", ".join(f"{k}={float(v):.5f}" for k, v in terms.items()))


if __name__ == "__main__":
    main(sys.argv[1])
