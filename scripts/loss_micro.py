"""Times DepthModel.compute_losses forward + backward (normals of gt and prediction included) on the HIP kernels
against the fp32 ATen restatement of the same rules (tests/loss_oracle.py evaluated in fp32 on the GPU), at B=8, K=7,
240x320 and 192x256, and counts the kernel launches of each.

    python scripts/loss_micro.py [--iters 20]
"""
import argparse
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import loss_oracle as lo  # noqa: E402
from simplerecon_amd import synthetic  # noqa: E402
from simplerecon_amd.depth_model import DepthModel  # noqa: E402


def batch(B, K, h, w):
    cur, src = synthetic.training_batch(B, K, h, w, seed=0, device="cuda")
    g = torch.Generator(device="cpu").manual_seed(0)
    log0 = (torch.log(torch.nan_to_num(cur["depth_b1hw"], nan=2.0)).cpu() + 0.05 * torch.randn(cur["depth_b1hw"].shape,
                                                                                             generator=g)).cuda()
    outs = {"log_depth_pred_s0_b1hw": log0}
    x = log0
    for i in range(1, 4):
        x = torch.nn.functional.avg_pool2d(x, 2, ceil_mode=True)
        outs[f"log_depth_pred_s{i}_b1hw"] = x
    outs["depth_pred_s0_b1hw"] = torch.exp(log0)
    return cur, src, outs


def hip_step(holder, cur, src, outs):
    leaves = {k: v.detach().requires_grad_(True) for k, v in outs.items()}
    c = dict(cur)
    o = dict(leaves)
    c["normals_b3hw"] = DepthModel.compute_normals(holder, c["depth_b1hw"], c["invK_s0_b44"])
    o["normals_pred_b3hw"] = DepthModel.compute_normals(holder, o["depth_pred_s0_b1hw"], c["invK_s0_b44"])
    DepthModel.compute_losses(holder, c, src, o)["loss"].backward()


def aten_step(cur, src, outs):
    leaves = {k: v.detach().requires_grad_(True) for k, v in outs.items()}
    c = dict(cur)
    o = dict(leaves)
    c["normals_b3hw"] = lo.normals(c["depth_b1hw"], c["invK_s0_b44"])
    o["normals_pred_b3hw"] = lo.normals(o["depth_pred_s0_b1hw"], c["invK_s0_b44"])
    lo.compute_losses(c, src, o)["loss"].backward()


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    lo.D = torch.float32   # the ATen restatement in fp32
    holder = types.SimpleNamespace(_loss_modules={})
    holder._losses_for = types.MethodType(DepthModel._losses_for, holder)
    for (B, K, h, w) in ((8, 7, 240, 320), (8, 7, 192, 256)):
        cur, src, outs = batch(B, K, h, w)
        t_hip = timed(lambda: hip_step(holder, cur, src, outs), a.iters)
        t_aten = timed(lambda: aten_step(cur, src, outs), a.iters)
        n_hip = launches(lambda: hip_step(holder, cur, src, outs))
        n_aten = launches(lambda: aten_step(cur, src, outs))
        print(f"B={B} K={K} {h}x{w}: HIP fwd+bwd {t_hip:.3f} ms ({n_hip} kernels) | "
              f"ATen fp32 {t_aten:.3f} ms ({n_aten} kernels)", flush=True)


if __name__ == "__main__":
    main()
