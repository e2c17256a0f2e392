"""A few training steps on synthetic data: synthetic.training_batch (ray-cast scenes with the reference's batch keys) ->
DepthModel.step("train") (forward, normals, the loss cocktail, all on HIP kernels) -> backward -> the HIP AdamW step
(simplerecon_amd.optim) with the reference's stepped LR schedule, through simplerecon_amd.training.fit.  It mirrors what the
reference's train.py does per step without Lightning, datasets or checkpoints.

    python examples/train_synthetic.py [--steps 5] [--batch 2] [--views 3] [--height 32] [--width 48] [--fp16]
                                       [--clip-grad-norm 1.0] [--loss-scaler hip|torch]

--fp16 runs the step under torch.autocast(float16) with the 16-bit MFMA convolutions (experimental.autocast_mfma16) and a
loss scaler: optim.LossScaler (--loss-scaler hip, the default: inf check, unscale and scale update inside the optimiser's
four launches) or torch.amp.GradScaler (torch), whose scale and found-inf flag the optimiser kernel reads on the device.
--clip-grad-norm clips the global gradient norm inside the step (Options.clip_grad_norm).  The gradient norm of every step
is printed beside the loss.  Weights start random and the batch is the same every step, so the loss only shows that the step
updates the weights.
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplerecon_amd import depth_model as dm  # noqa: E402
from simplerecon_amd import optim, synthetic, training  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--views", type=int, default=3, help="source views per frame")
    ap.add_argument("--height", type=int, default=32, help="depth-map height (the images are twice as large)")
    ap.add_argument("--width", type=int, default=48)
    ap.add_argument("--fp16", action="store_true")
    ap.add_argument("--clip-grad-norm", type=float, default=0.0, help="clip the global gradient norm to this value (0: off)")
    ap.add_argument("--loss-scaler", choices=("hip", "torch"), default="hip", help="the scaler of --fp16")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "the training path runs on HIP kernels: a GPU is needed"
    dev = "cuda:0"
    opts = dm.default_options(image_width=2 * args.width, image_height=2 * args.height, model_num_views=args.views + 1,
                              matching_num_depth_bins=8, clip_grad_norm=args.clip_grad_norm)
    model = dm.DepthModel(opts)
    for i, m in enumerate((model.encoder, model.matching_model, model.cost_volume_net, model.depth_decoder,
                           model.cost_volume.mlp)):
        synthetic.seeded_fill_(m, seed=11 + i)
    model = model.to(dev)
    batch = synthetic.training_batch(args.batch, args.views, args.height, args.width, seed=6, device=dev)
    cfg = model.configure_optimizers()          # optim.AdamW(lr, wd) + LambdaLR(1 / 0.1 / 0.01 at opts.lr_steps)
    optimizer, scheduler = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
    optimizer.grad_stats = True                 # the norms are wanted also where nothing clips or scales
    scaler = None
    if args.fp16:
        scaler = optim.LossScaler() if args.loss_scaler == "hip" else torch.amp.GradScaler("cuda")
    losses, norms = [], []

    def on_step(step, loss):                    # device tensors: no synchronisation per step
        losses.append(loss)
        norms.append(optimizer.grad_norm.clone())      # (the optimiser overwrites it at the next step)

    def batches():
        while True:
            yield batch
    steps = training.fit(model, batches(), args.steps, optimizer=optimizer, scheduler=scheduler, scaler=scaler,
                         autocast_dtype=torch.float16 if args.fp16 else None, mfma16=2 if args.fp16 else None,
                         on_step=on_step)
    for step, (loss, norm) in enumerate(zip(losses, norms), 1):
        print(f"step {step}: loss {float(loss):.5f}  gradient norm {float(norm):.4g}")
    print(f"{steps} steps, lr {scheduler.get_last_lr()[0]:g}" + (f", loss scale {scaler.get_scale():g}" if scaler else ""))


if __name__ == "__main__":
    main()
