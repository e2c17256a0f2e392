"""The 16-bit MFMA convolution (sr_conv16_nhwc_fwd) against the path the same fp16 / bf16 tensors take without it, on the conv-stack
layer shapes of profiles/r06_layer_tables.txt at batch 8 and 2 -- the table sr_conv16_prefers is fitted on (profiles/r07_conv16.txt).

Per shape and dtype, in ONE process, alternating rounds of back-to-back launches between device events, after a warm-up:
  kernel   sr_conv16_nhwc_fwd alone on a pre-packed weight: time, achieved FLOP/s (direct-convolution FLOPs of the shape), the
           floor max(FLOPs / 16-bit matrix peak, bytes / HBM rate) and which of the two bounds it;
  new      autograd_ops._conv_raw_io with MFMA16 = 2: what a training step launches (weight cast + pack on the fly, then the kernel);
  parent   autograd_ops._conv_raw_io with MFMA16 = 0: sr_conv3x3_wino_io_nhwc_fwd / sr_pw_conv_io_nhwc_fwd on their fp32 packed
           weight, or boundary conversion around the fp32 direct kernel (3x3 / stride 2);
  spread   (max - min) / median over the rounds of identical launches, the larger of the two paths';
  rule     what sr_conv16_prefers answers for the shape, and whether new beat parent by more than the spread.
    python scripts/conv16_micro.py [rounds] [launches per round]"""
import os
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from simplerecon_amd import _lib, autograd_ops, ops

DEV = torch.device("cuda", 0)
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
N = int(sys.argv[2]) if len(sys.argv) > 2 else 20
PEAK16, HBM = 2.5e15, 6.29e12     # dense 16-bit matrix peak (spec), measured HBM copy rate
# (Ci, H, W, Co, k, stride) at batch 8 (profiles/r06_layer_tables.txt); batch 2 is run on the same list
LAYERS = [(64, 240, 320, 64, 3, 1), (64, 120, 160, 64, 3, 1), (64, 60, 80, 64, 3, 1), (128, 60, 80, 128, 3, 1), (256, 30, 40, 128, 3, 1),
          (128, 60, 80, 64, 1, 1), (256, 30, 40, 128, 1, 1),
          (24, 240, 320, 96, 3, 2), (48, 120, 160, 192, 3, 2), (64, 120, 160, 128, 3, 2), (128, 60, 80, 256, 3, 2), (256, 30, 40, 384, 3, 2)]
IO = {torch.float16: 1, torch.bfloat16: 2}


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
    print(f"# {'(B,Ci,H,W,Co,k,s)':30s} {'dtype':5s} {'kernel us':>9s} {'TF/s':>6s} {'floor us':>8s} {'bound':>6s} {'new us':>8s} "
          f"{'parent us':>9s} {'spread':>6s} {'new/parent':>10s} {'prefers':>7s} {'beats':>5s}")
    for B in (8, 2):
        for ci, H, W, co, k, s in LAYERS:
            ho, wo = ops.conv_out_hw(H, W, s, k)
            flops = 2.0 * B * ho * wo * co * ci * k * k
            nbytes = 2.0 * (B * H * W * ci + B * ho * wo * co + co * ci * k * k)
            floor_c, floor_m = flops / PEAK16, nbytes / HBM
            for dt in (torch.bfloat16, torch.float16):
                g = torch.Generator().manual_seed(ci + co + H)
                x = torch.randn((B, ci, H, W), generator=g).to(DEV).to(dt).contiguous(memory_format=torch.channels_last)
                conv = torch.nn.Conv2d(ci, co, k, stride=s, padding=k // 2).to(DEV)
                weight, bias = conv.weight.detach(), conv.bias.detach()
                wp = torch.empty(lib.sr_conv16_packed_weight_bytes(co, ci, k), dtype=torch.uint8, device=DEV)
                _lib.call("sr_conv16_pack_weights", DEV, weight, co, ci, k, IO[dt], wp)
                out = torch.empty((B, co, ho, wo), dtype=dt, device=DEV, memory_format=torch.channels_last)

                def kernel():
                    _lib.call("sr_conv16_nhwc_fwd", DEV, x, *ops._strides(x), wp, bias, None, 0, 0, out, *ops._strides(out), B, H, W,
                              ci, co, k, s, 0.2, IO[dt], IO[dt])

                def path(mode):
                    def run():
                        autograd_ops.MFMA16 = mode
                        return autograd_ops._conv_raw_io(x, weight, bias, s, None, 0.2, None)
                    return run
                new, parent = path(2), path(0)
                with torch.inference_mode():
                    for f in (kernel, new, parent):
                        for _ in range(3):
                            f()
                    torch.cuda.synchronize()
                    err = float((new().float() - parent().float()).abs().max())
                    t = {"kernel": [], "new": [], "parent": []}
                    for _ in range(ROUNDS):
                        for name, f in (("kernel", kernel), ("new", new), ("parent", parent)):
                            t[name].append(timed(f))
                autograd_ops.MFMA16 = 0
                med = {n: float(np.median(v)) for n, v in t.items()}
                spread = max((max(v) - min(v)) / med[n] for n, v in t.items() if n != "kernel")
                beats = med["new"] < med["parent"] * (1.0 - spread)
                print(f"  {str((B, ci, H, W, co, k, s)):30s} {'bf16' if dt == torch.bfloat16 else 'fp16':5s} {med['kernel'] * 1e6:9.1f} "
                      f"{flops / med['kernel'] / 1e12:6.1f} {max(floor_c, floor_m) * 1e6:8.1f} {'matrix' if floor_c > floor_m else 'HBM':>6s} "
                      f"{med['new'] * 1e6:8.1f} {med['parent'] * 1e6:9.1f} {spread:6.3f} {med['new'] / med['parent']:10.3f} "
                      f"{lib.sr_conv16_prefers(B, H, W, ci, co, k, s):7d} {'yes' if beats else 'no':>5s}   max |new - parent| {err:.3g}",
                      flush=True)


if __name__ == "__main__":
    main()
