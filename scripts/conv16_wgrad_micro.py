"""The 16-bit weight gradient (sr_act_bwd_bias16_nhwc + sr_conv16_wgrad_nhwc) against the path the same fp16 / bf16 tensors take
without it, on the conv-stack layer shapes of profiles/r06_layer_tables.txt at batch 8 and 2 -- the table sr_conv16_wgrad_prefers
is to be fitted on (profiles/r08_conv16_wgrad.txt).

Per shape and dtype, in ONE process, alternating rounds of back-to-back launches between device events, after a warm-up, on a saved
16-bit input x, a saved 16-bit output and a 16-bit arriving gradient g (LeakyReLU 0.2, with a bias gradient):
  kernel   sr_conv16_wgrad_nhwc alone (both launches: slabs + ordered reduce): time and achieved FLOP/s (2 B Ho Wo Co Ci k k);
  new      sr_act_bwd_bias16_nhwc + sr_conv16_wgrad_nhwc on the 16-bit tensors;
  parent   what _ConvBiasAct.backward does for such a layer without the switch: .float() copies of x, out and g,
           sr_act_bwd_bias_nhwc + sr_conv_wgrad_nhwc in fp32, then .to(dtype) of the post-activation gradient;
  spread   (max - min) / median over the rounds of identical launches, the larger of the two paths';
  rule     what sr_conv16_wgrad_prefers answers for the shape, and whether new beat parent by more than the spread;
  max |new - parent| of dW (the parent multiplies the same 16-bit values in fp32: the two differ by summation order only).
    python scripts/conv16_wgrad_micro.py [rounds] [launches per round]"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from simplerecon_amd import _lib, ops

DEV = torch.device("cuda", 0)
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N = int(sys.argv[2]) if len(sys.argv) > 2 else 10
# (Ci, H, W, Co, k, stride) at batch 8 (profiles/r06_layer_tables.txt); batch 2 is run on the same list
LAYERS = [(64, 240, 320, 64, 3, 1), (64, 120, 160, 64, 3, 1), (64, 60, 80, 64, 3, 1), (128, 60, 80, 128, 3, 1), (256, 30, 40, 128, 3, 1),
          (128, 60, 80, 64, 1, 1), (256, 30, 40, 128, 1, 1),
          (24, 240, 320, 96, 3, 2), (48, 120, 160, 192, 3, 2), (64, 120, 160, 128, 3, 2), (128, 60, 80, 256, 3, 2), (256, 30, 40, 384, 3, 2)]
IO = {torch.float16: 1, torch.bfloat16: 2}
SLOPE = 0.2


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(N):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / N


def main():
    lib = _lib.lib()
    print(f"# rounds {ROUNDS} x {N} launches, alternating; times are medians over the rounds; spread = (max - min) / median")
    print(f"# {'(B,Ci,H,W,Co,k,s)':30s} {'dtype':5s} {'kernel us':>9s} {'TF/s':>6s} {'new us':>8s} {'parent us':>9s} {'spread':>6s} "
          f"{'new/parent':>10s} {'prefers':>7s} {'beats':>5s}")
    for B in (8, 2):
        for ci, H, W, co, k, s in LAYERS:
            ho, wo = ops.conv_out_hw(H, W, s, k)
            px = B * ho * wo
            flops = 2.0 * px * co * ci * k * k
            for dt in (torch.bfloat16, torch.float16):
                gen = torch.Generator().manual_seed(ci + co + H)
                x = torch.randn((B, ci, H, W), generator=gen).to(DEV).to(dt).contiguous(memory_format=torch.channels_last)
                out = torch.randn((B, co, ho, wo), generator=gen).to(DEV).to(dt).contiguous(memory_format=torch.channels_last)
                g = (torch.randn((B, co, ho, wo), generator=gen) * px ** -0.5).to(DEV).to(dt).contiguous(memory_format=torch.channels_last)
                gp16 = torch.empty_like(g)
                dw16 = torch.empty((co, ci, k, k), dtype=torch.float32, device=DEV)
                dw32 = torch.empty_like(dw16)
                db16 = torch.empty((co,), dtype=torch.float32, device=DEV)
                db32 = torch.empty_like(db16)
                n_w16 = lib.sr_conv16_wgrad_workspace_bytes(B, H, W, ci, co, k, s)
                n_w32 = lib.sr_conv_wgrad_workspace_bytes(B, H, W, ci, co, k, s)
                n_b16 = lib.sr_act_bwd_bias16_workspace_bytes(px, co)
                n_b32 = lib.sr_act_bwd_bias_workspace_bytes(px, co)
                ws_w = torch.empty(max(n_w16, n_w32) // 4, dtype=torch.float32, device=DEV)
                ws_b = torch.empty(max(n_b16, n_b32) // 4, dtype=torch.float32, device=DEV)

                def kernel():
                    _lib.call("sr_conv16_wgrad_nhwc", DEV, x, *ops._strides(x), gp16, *ops._strides(gp16), dw16, B, H, W, ci, co, k, s,
                              IO[dt], ws_w, n_w16)

                def new():
                    _lib.call("sr_act_bwd_bias16_nhwc", DEV, g, IO[dt], out, gp16, db16, px, co, SLOPE, IO[dt], ws_b, n_b16)
                    kernel()
                    return gp16

                def parent():
                    x32, o32, g32 = x.float(), out.float(), g.float()
                    gp = torch.empty_like(g32)
                    _lib.call("sr_act_bwd_bias_nhwc", DEV, g32, o32, gp, db32, px, co, SLOPE, ws_b, n_b32)
                    _lib.call("sr_conv_wgrad_nhwc", DEV, x32, *ops._strides(x32), gp, *ops._strides(gp), dw32, B, H, W, ci, co, k, s,
                              ws_w, n_w32)
                    return gp.to(dt)

                with torch.inference_mode():
                    for f in (new, kernel, parent):
                        for _ in range(2):
                            f()
                    torch.cuda.synchronize()
                    err = float((dw16 - dw32).abs().max())
                    scale = float(dw32.abs().max())
                    t = {"kernel": [], "new": [], "parent": []}
                    for _ in range(ROUNDS):
                        for name, f in (("kernel", kernel), ("new", new), ("parent", parent)):
                            t[name].append(timed(f))
                med = {n: float(np.median(v)) for n, v in t.items()}
                spread = max((max(v) - min(v)) / med[n] for n, v in t.items() if n != "kernel")
                beats = med["new"] < med["parent"] * (1.0 - spread)
                print(f"  {str((B, ci, H, W, co, k, s)):30s} {'bf16' if dt == torch.bfloat16 else 'fp16':5s} {med['kernel'] * 1e6:9.1f} "
                      f"{flops / med['kernel'] / 1e12:6.1f} {med['new'] * 1e6:8.1f} {med['parent'] * 1e6:9.1f} {spread:6.3f} "
                      f"{med['new'] / med['parent']:10.3f} {lib.sr_conv16_wgrad_prefers(B, H, W, ci, co, k, s):7d} "
                      f"{'yes' if beats else 'no':>5s}   max |new - parent| {err:.3g} of max |dW| {scale:.3g}", flush=True)
                del x, out, g, gp16, ws_w, ws_b


if __name__ == "__main__":
    main()
