"""The optimiser step on the full model's parameter set, and the whole training step with the update in it.

Part "optim": optim.AdamW.step() (two launches) against torch.optim.AdamW with foreach=False, foreach=True and fused=True, in ONE
process, alternating, on DepthModel(default_options())'s 778 parameter tensors with random gradients.  Per step: HIP-event time
around step() with the device idle at the start (what the device spends), and the host clock over back-to-back steps that end in
a synchronise (what a training loop pays: the larger of host and device work).  Median and spread = (max - min) / median over the
steps.  The floor: the step moves 28 bytes per parameter; a device-to-device copy of the same number of bytes is timed beside it.

Part "train": scripts/train_step_mfma16.py's model, inputs and loss (batch 2, 7 views, 640x480, 64 planes) -- forward + backward
alone, + optim.AdamW, + torch.optim.AdamW(fused=True) --, in fp32 and under bf16 autocast_mfma16(mode=2, wgrad=2), alternating; and
the cost of packing every weight again after an update: the first eval forward after a step minus a forward with warm caches.

    python scripts/optim_step_bench.py [optim|train|all] [steps]"""
import contextlib
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


def bench_optim():
    shapes = [tuple(p.shape) for p in dm.DepthModel(dm.default_options()).parameters()]
    numel = sum(int(np.prod(s)) for s in shapes)
    print(f"# {len(shapes)} parameter tensors, {numel} elements, {28 * numel / 1e9:.3f} GB per step (28 B per element)")
    g = torch.Generator(device=dev).manual_seed(0)
    grads = [torch.randn(s, device=dev, generator=g) * 1e-3 for s in shapes]

    def params():
        return [torch.randn(s, device=dev, generator=g).requires_grad_() for s in shapes]
    kw = dict(lr=1e-4, weight_decay=1e-4)
    variants = [("optim.AdamW (HIP, 2 launches)", optim.AdamW, {}),
                ("torch AdamW fused=True", torch.optim.AdamW, dict(fused=True)),
                ("torch AdamW foreach=True", torch.optim.AdamW, dict(foreach=True)),
                ("torch AdamW foreach=False", torch.optim.AdamW, dict(foreach=False))]
    opts = []
    for name, cls, extra in variants:
        ps = params()
        for p, gr in zip(ps, grads):
            p.grad = gr
        opts.append((name, cls(ps, **kw, **extra)))
    for _, o in opts:          # warm-up: state, tables, code objects
        for _ in range(3):
            o.step()
    torch.cuda.synchronize()
    ev_times = {name: [] for name, _ in opts}
    wall = {name: [] for name, _ in opts}
    rounds, per = 4, max(1, STEPS // 4)
    for _ in range(rounds):
        for name, o in opts:
            for _ in range(per):
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                o.step()
                b.record()
                b.synchronize()
                ev_times[name].append(a.elapsed_time(b) * 1e-3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(per):
                o.step()
            torch.cuda.synchronize()
            wall[name].append((time.perf_counter() - t0) / per)
    # the floor: a copy that moves as many bytes as the step (14 B read + 14 B written per parameter)
    n = 28 * numel // 2 // 4
    src, dst = torch.empty(n, device=dev), torch.empty(n, device=dev)
    copies = []
    for i in range(13):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        if i >= 3:
            copies.append(a.elapsed_time(b) * 1e-3)
    copy_t = float(np.median(copies))
    bw = 8 * n / copy_t
    print(f"# device copy of the same {8 * n / 1e9:.3f} GB: {copy_t * 1e3:.3f} ms = {bw / 1e12:.2f} TB/s")
    print(f"# {rounds} alternating rounds x {per} steps; 'events' = HIP events around one step() on an idle device, 'loop' = host "
          f"clock per step over {per} back-to-back steps ending in a synchronise")
    for name, _ in opts:
        ev = float(np.median(ev_times[name]))
        print(f"  {name:32s} events {stats(ev_times[name])}   loop {stats(wall[name])}   copy time / events = {copy_t / ev:5.2f}",
              flush=True)


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
    updates = {"no update": None,
               "optim.AdamW": optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-4),
               "torch AdamW fused": torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-4, fused=True)}
    precisions = {"fp32": (False, contextlib.nullcontext),
                  "bf16 autocast_mfma16(2, wgrad=2)": (True, lambda: experimental.autocast_mfma16(mode=2, wgrad=2))}

    def step(autocast, opt):
        model.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            out = model("train", cur, src)
            loss = sum(out[f"log_depth_pred_s{i}_b1hw"].float().abs().mean() for i in range(4))
        loss.backward()
        if opt is not None:
            opt.step()
    configs = [(p, u) for p in precisions for u in updates]
    times = {c: [] for c in configs}
    for p, u in configs:
        with precisions[p][1]():
            for _ in range(2):
                step(precisions[p][0], updates[u])
    rounds, per = 3, 4
    for _ in range(rounds):
        for p, u in configs:
            with precisions[p][1]():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(per):
                    step(precisions[p][0], updates[u])
                torch.cuda.synchronize()
                times[(p, u)].append((time.perf_counter() - t0) / per)
    print(f"# training step: batch {B}, {K} views, {D} planes, {W}x{H}, encoders trained; {rounds} alternating rounds x {per} steps, "
          f"host clock around steps ending in a synchronise")
    for p, u in configs:
        print(f"  {p:34s} {u:20s} {stats(times[(p, u)])}", flush=True)
    # packing every weight again after an update
    model.eval()
    args = (cur["image_b3hw"], src["image_b3hw"], src["cam_T_world_b44"] @ cur["world_T_cam_b44"].unsqueeze(1),
            cur["cam_T_world_b44"].unsqueeze(1) @ src["world_T_cam_b44"], src["K_s1_b44"], cur["invK_s1_b44"])

    def forward():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            model.forward_tensors(*args)
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    opt = updates["optim.AdamW"]      # (gradients of the last training step are still in place)
    first, warm = [], []
    forward()
    for _ in range(5):
        opt.step()
        first.append(forward())
        warm += [forward(), forward()]
    print(f"# eval forward, batch {B}: first after an update {stats(first)}; warm caches {stats(warm)}; "
          f"re-pack of every weight = {(np.median(first) - np.median(warm)) * 1e3:.3f} ms per step (open item: not addressed here)")


if PART in ("optim", "all"):
    bench_optim()
if PART in ("train", "all"):
    bench_train()
