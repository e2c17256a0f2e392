"""The training step around DepthModel.step: zero_grad, forward + backward, the HIP optimiser step (optim.AdamW), loss
scaler, LR schedule -- the plain loop the reference gets from Lightning (train.py; depth_model.py:502-633), without
Lightning, logging or checkpoint I/O.

    cfg = model.configure_optimizers()
    opt, sched = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
    for batch in loader:
        loss = training.train_step(model, batch, opt, sched)        # a 0-dim device tensor: no host synchronisation

Gradient clipping is the optimiser's (Options.clip_grad_norm -> optim.AdamW(max_grad_norm=...)); after a step
`optimizer.grad_norm` holds the global gradient norm on the device, for an on_step callback to read.  The scaler is a
torch.amp.GradScaler or an optim.LossScaler (inf check, unscale and scale update inside the optimiser's four launches).

Not provided: HIP-graph capture of the step."""
import contextlib

import torch

DEFAULT_LR_STEPS = (70000, 80000)   # options.py:82-104


def lr_factor(step, lr_steps=DEFAULT_LR_STEPS):
    """The reference's stepped schedule (depth_model.py:624-630): 1 before lr_steps[0], 0.1 before lr_steps[1], 0.01
    from there on.  `step` counts optimiser steps (LambdaLR's last_epoch with interval "step")."""
    if step < lr_steps[0]:
        return 1
    if step < lr_steps[1]:
        return 0.1
    return 0.01


def train_step(model, batch, optimizer, scheduler=None, scaler=None, autocast_dtype=None, mfma16=None):
    """One optimisation step on `batch` = (cur_data, src_data); returns the detached loss without synchronising.

    autocast_dtype: torch.float16 / torch.bfloat16 runs forward and backward inside torch.autocast; mfma16 (1 or 2, with an
    autocast_dtype) adds experimental.autocast_mfma16(mode=mfma16) around both, as the data gradient reads the switch.
    scaler: a torch.amp.GradScaler or an optim.LossScaler (fp16 needs one): the loss is scaled, the step goes through
    scaler.step, which hands optim.AdamW the scale and the found-inf flag on the device, then scaler.update()."""
    if mfma16 and autocast_dtype is None:
        raise ValueError("mfma16 needs an autocast_dtype (the 16-bit MFMA convolutions run under torch.autocast)")
    optimizer.zero_grad()
    with contextlib.ExitStack() as stack:
        if mfma16:
            from . import experimental
            stack.enter_context(experimental.autocast_mfma16(mode=mfma16))
        with torch.autocast("cuda", dtype=autocast_dtype, enabled=autocast_dtype is not None):
            loss = model.step("train", batch)
        (scaler.scale(loss) if scaler is not None else loss).backward()   # inside the mfma16 block
    if scaler is not None:
        scaler.step(optimizer)
        scaler.update()
    else:
        optimizer.step()
    if scheduler is not None:
        scheduler.step()
    return loss.detach()


def fit(model, batches, max_steps, optimizer=None, scheduler=None, scaler=None, autocast_dtype=None, mfma16=None,
        on_step=None):
    """train_step over the iterable `batches` until it ends or `max_steps` steps ran; returns the number of steps.
    Without an `optimizer`, model.configure_optimizers() supplies it and the schedule.  on_step(step, loss), if given,
    runs after every step with the loss still on the device."""
    steps = 0
    if max_steps <= 0:
        return steps
    if optimizer is None:
        cfg = model.configure_optimizers()
        optimizer, scheduler = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
    model.train()
    for batch in batches:
        loss = train_step(model, batch, optimizer, scheduler, scaler, autocast_dtype, mfma16)
        steps += 1
        if on_step is not None:
            on_step(steps, loss)
        if steps >= max_steps:
            break
    return steps
