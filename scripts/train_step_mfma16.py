"""The whole training step (scripts/train_step_micro.py's model, inputs and loss) in five configurations, side by side in ONE process,
alternating: fp32; bf16 autocast with the 16-bit switches off (fp32 kernels); HALF_IO + STORE_HALF; experimental.autocast_mfma16
(HALF_IO + STORE_HALF + the 16-bit MFMA convolutions where SR_TRAIN_MFMA16_MODE, default 1 = the measured rule, selects them); the
same with the 16-bit weight gradient and cast-free elementwise backward (wgrad = SR_TRAIN_MFMA16_WGRAD, default 2 = every supported
layer whose forward ran on the 16-bit kernel).
Time per step (host clock around steps that end in a device synchronise) and peak memory per configuration.
    [SR_TRAIN_AUTOCAST=bf16|fp16] [SR_TRAIN_MFMA16_MODE=1|2] [SR_TRAIN_MFMA16_WGRAD=1|2] python scripts/train_step_mfma16.py [batch] [views] [rounds] [steps]"""
import contextlib
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from simplerecon_amd import autograd_ops, depth_model as dm, experimental, synthetic

B = int(sys.argv[1]) if len(sys.argv) > 1 else 2
K = int(sys.argv[2]) if len(sys.argv) > 2 else 7
ROUNDS = int(sys.argv[3]) if len(sys.argv) > 3 else 3
STEPS = int(sys.argv[4]) if len(sys.argv) > 4 else 3
AMP = os.environ.get("SR_TRAIN_AUTOCAST", "bf16")
AMP_DT = {"fp16": torch.float16, "bf16": torch.bfloat16}[AMP]
MODE = int(os.environ.get("SR_TRAIN_MFMA16_MODE", "1"))
WGRAD = int(os.environ.get("SR_TRAIN_MFMA16_WGRAD", "2"))
D, H, W = 64, 480, 640
dev = torch.device("cuda", 0)
opts = dm.default_options(image_width=W, image_height=H, model_num_views=K + 1, matching_num_depth_bins=D)
model = dm.DepthModel(opts)
synthetic.seeded_fill_(model.encoder, seed=6, gain=1.0)
for i, m in enumerate((model.matching_model, model.cost_volume_net, model.depth_decoder, model.cost_volume.mlp)):
    synthetic.seeded_fill_(m, seed=40 + i)
model = model.to(dev).train()
inp = synthetic.cost_volume_inputs(B, K, 16, H // 4, W // 4, seed=6, device=dev)
rng = np.random.default_rng(1)
eye = torch.eye(4, device=dev).expand(B, 4, 4).contiguous()
cur = {"image_b3hw": torch.from_numpy(rng.standard_normal((B, 3, H, W)).astype("float32")).to(dev),
       "invK_s1_b44": inp["cur_invK"], "cam_T_world_b44": eye, "world_T_cam_b44": eye}
src = {"image_b3hw": torch.from_numpy(rng.standard_normal((B, K, 3, H, W)).astype("float32")).to(dev),
       "K_s1_b44": inp["src_Ks"], "cam_T_world_b44": inp["src_extrinsics"], "world_T_cam_b44": inp["src_poses"]}


@contextlib.contextmanager
def switches(half_io, store_half):
    saved = (autograd_ops.HALF_IO, autograd_ops.STORE_HALF, autograd_ops.MFMA16, autograd_ops.MFMA16_WGRAD)
    autograd_ops.HALF_IO, autograd_ops.STORE_HALF, autograd_ops.MFMA16, autograd_ops.MFMA16_WGRAD = half_io, store_half, 0, 0
    try:
        yield
    finally:
        autograd_ops.HALF_IO, autograd_ops.STORE_HALF, autograd_ops.MFMA16, autograd_ops.MFMA16_WGRAD = saved


CONFIGS = [("fp32", False, lambda: switches(False, False)),
           (f"{AMP} autocast, switches off", True, lambda: switches(False, False)),
           (f"{AMP} HALF_IO + STORE_HALF", True, lambda: switches(True, True)),
           (f"{AMP} autocast_mfma16(mode={MODE})", True, lambda: experimental.autocast_mfma16(mode=MODE)),
           (f"{AMP} autocast_mfma16(mode={MODE}, wgrad={WGRAD})", True, lambda: experimental.autocast_mfma16(mode=MODE, wgrad=WGRAD))]


def step(autocast):
    model.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=AMP_DT, enabled=autocast):
        out = model("train", cur, src)
        loss = sum(out[f"log_depth_pred_s{i}_b1hw"].float().abs().mean() for i in range(4))
    loss.backward()
    return float(loss.detach())


times = {name: [] for name, _, _ in CONFIGS}
peak, losses = {}, {}
for name, autocast, ctx in CONFIGS:          # warm-up, and the peak memory of each configuration on its own
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats()
    with ctx():
        for _ in range(2):
            losses[name] = step(autocast)
    torch.cuda.synchronize()
    peak[name] = torch.cuda.max_memory_allocated() / 2 ** 30
for _ in range(ROUNDS):
    for name, autocast, ctx in CONFIGS:
        with ctx():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(STEPS):
                step(autocast)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / STEPS)
print(f"# batch {B}, {K} views, 64 planes, 640x480, encoders trained; {ROUNDS} alternating rounds x {STEPS} steps; "
      f"spread = (max - min) / median over the rounds")
for name, _, _ in CONFIGS:
    t = times[name]
    print(f"  {name:48s} {np.median(t) * 1e3:7.1f} ms/step  spread {(max(t) - min(t)) / np.median(t):.3f}  peak {peak[name]:.2f} GiB  "
          f"loss {losses[name]:.5f}", flush=True)
