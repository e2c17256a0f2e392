"""Gradient statistics, clipping and the loss scaler on the full model's parameter set, against torch's own path in the same run.

Part "optim": DepthModel(default_options())'s 778 parameter tensors with random gradients, the method of
scripts/optim_step_bench.py: variants in ONE process, alternating rounds; per step HIP events around the call with the device
idle at the start, and the host clock over back-to-back calls that end in a synchronise.  Median and spread = (max - min) /
median.
  * the statistics pass alone (sr_grad_stats, two launches): device time over queued calls, bytes read per second, beside a
    device copy that moves the same number of bytes;
  * scaler.step + update: torch.amp.GradScaler against optim.LossScaler, both around optim.AdamW;
  * clipping: torch.nn.utils.clip_grad_norm_ + step and optim.clip_grad_norm_ + step against the fused clipped step.

Part "train": scripts/optim_step_bench.py's model, inputs and loss (batch 2, 7 views, 640x480, 64 planes) under fp16 autocast with
autocast_mfma16(mode=2): torch.amp.GradScaler, optim.LossScaler, and optim.LossScaler with max_grad_norm=1, alternating.

    python scripts/grad_stats_bench.py [optim|train|all] [steps]"""
import os
import sys
import time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from simplerecon_amd import depth_model as dm, experimental, optim, synthetic

PART = sys.argv[1] if len(sys.argv) > 1 else "all"
STEPS = int(sys.argv[2]) if len(sys.argv) > 2 else 24
dev = torch.device("cuda", 0)
assert torch.cuda.is_available(), "needs a GPU"


def stats(t):
    t = np.asarray(t) * 1e3
    return f"{np.median(t):8.3f} ms  spread {(t.max() - t.min()) / np.median(t):5.2f}"


def event_time(fn, repeat=1):
    """HIP-event seconds per call of `fn`, `repeat` calls queued between the events, the device idle at the start."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeat):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3 / repeat


def bench_optim():
    shapes = [tuple(p.shape) for p in dm.DepthModel(dm.default_options()).parameters()]
    numel = sum(int(np.prod(s)) for s in shapes)
    print(f"# {len(shapes)} parameter tensors, {numel} elements, {4 * numel / 1e9:.3f} GB of gradients")
    g = torch.Generator(device=dev).manual_seed(0)
    grads = [torch.randn(s, device=dev, generator=g) * 1e-3 for s in shapes]
    kw = dict(lr=1e-4, weight_decay=1e-4)

    def optimiser(**extra):
        ps = [torch.randn(s, device=dev, generator=g).requires_grad_() for s in shapes]
        for p, gr in zip(ps, grads):
            p.grad = gr
        return ps, optim.AdamW(ps, **kw, **extra)

    def scaled(scaler, opt):
        def call():
            scaler.step(opt)
            scaler.update()
        return call

    def clip_then_step(clip, ps, opt):
        def call():
            clip(ps, 1.0)
            opt.step()
        return call
    torch_scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10)
    torch_scaler.scale(torch.zeros((), device=dev))
    variants = [("optim.AdamW (2 launches)", optimiser()[1].step),
                ("optim.AdamW grad_stats=True (4)", optimiser(grad_stats=True)[1].step),
                ("GradScaler.step + update", scaled(torch_scaler, optimiser()[1])),
                ("LossScaler.step + update", scaled(optim.LossScaler(init_scale=2.0 ** 10), optimiser()[1])),
                ("torch clip_grad_norm_ + step", clip_then_step(torch.nn.utils.clip_grad_norm_, *optimiser())),
                ("optim.clip_grad_norm_ + step", clip_then_step(optim.clip_grad_norm_, *optimiser())),
                ("optim.AdamW max_grad_norm=1 (4)", optimiser(max_grad_norm=1.0)[1].step)]
    for _, fn in variants:          # warm-up: state, tables, code objects
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ev_times = {name: [] for name, _ in variants}
    wall = {name: [] for name, _ in variants}
    rounds, per = 4, max(1, STEPS // 4)
    for _ in range(rounds):
        for name, fn in variants:
            for _ in range(per):
                ev_times[name].append(event_time(fn))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(per):
                fn()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) / per)
    # the statistics pass alone, and a copy that moves as many bytes as it reads
    ps, opt = optimiser(grad_stats=True)
    opt.step()
    tables = opt._plan["tables"]
    n = numel // 2
    src, dst = torch.empty(n, device=dev), torch.empty(n, device=dev)
    for _ in range(3):
        tables.stats()
        dst.copy_(src)
    pass_t = [event_time(tables.stats, repeat=20) for _ in range(9)]
    copy_t = [event_time(lambda: dst.copy_(src), repeat=20) for _ in range(9)]
    one_t = [event_time(tables.stats) for _ in range(9)]
    p, c = float(np.median(pass_t)), float(np.median(copy_t))
    print(f"# statistics pass alone (sr_grad_stats, both launches), 20 queued calls between HIP events: {stats(pass_t)} per call = "
          f"{4 * numel / p / 1e12:.2f} TB/s read")
    print(f"# device copy that moves the same {8 * n / 1e9:.3f} GB, measured the same way:              {stats(copy_t)} per call = "
          f"{8 * n / c / 1e12:.2f} TB/s; pass rate / copy rate = {c / p:.2f}")
    print(f"# statistics pass alone, one call on an idle device (HIP events):                        {stats(one_t)}")
    print(f"# {rounds} alternating rounds x {per} steps; 'events' = HIP events around one call on an idle device, 'loop' = host "
          f"clock per call over {per} back-to-back calls ending in a synchronise")
    for name, _ in variants:
        print(f"  {name:34s} events {stats(ev_times[name])}   loop {stats(wall[name])}", flush=True)


def bench_train():
    B, K, D, H, W = 2, 7, 64, 480, 640
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
    kw = dict(lr=1e-4, weight_decay=1e-4)
    torch_scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10)
    configs = {"torch.amp.GradScaler": (torch_scaler, optim.AdamW(model.parameters(), **kw)),
               "optim.LossScaler": (optim.LossScaler(init_scale=2.0 ** 10), optim.AdamW(model.parameters(), **kw)),
               "optim.LossScaler, max_grad_norm=1": (optim.LossScaler(init_scale=2.0 ** 10),
                                                     optim.AdamW(model.parameters(), max_grad_norm=1.0, **kw))}

    def step(scaler, opt):
        model.zero_grad(set_to_none=True)
        with experimental.autocast_mfma16(mode=2):
            with torch.autocast("cuda", dtype=torch.float16):
                out = model("train", cur, src)
                loss = sum(out[f"log_depth_pred_s{i}_b1hw"].float().abs().mean() for i in range(4))
            scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()
    times = {c: [] for c in configs}
    for c in configs:
        for _ in range(2):
            step(*configs[c])
    rounds, per = 3, 4
    for _ in range(rounds):
        for c in configs:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(per):
                step(*configs[c])
            torch.cuda.synchronize()
            times[c].append((time.perf_counter() - t0) / per)
    print(f"# training step: batch {B}, {K} views, {D} planes, {W}x{H}, fp16 autocast_mfma16(mode=2), optim.AdamW; {rounds} alternating "
          f"rounds x {per} steps, host clock around steps ending in a synchronise")
    for c in configs:
        print(f"  {c:36s} {stats(times[c])}   scale at the end {configs[c][0].get_scale():g}", flush=True)
    last = configs["optim.LossScaler, max_grad_norm=1"][1]
    print(f"# last clipped step: gradient norm {float(last.grad_norm):.4g}, coefficient {float(last.clip_coef):.4g}, "
          f"found_inf {float(last.found_inf_last):g}")


if PART in ("optim", "all"):
    bench_optim()
if PART in ("train", "all"):
    bench_train()
