"""Experiment switches of the HIP library, as context managers.  Nothing here is on a default path.

`split_precision("f16")` turns on the two fenced split-precision kernels for the calls made inside
the block: the metadata-MLP sweep's layers 1-2 and the Winograd 3x3 convolutions then multiply on the 16-bit matrix pipe --
every fp32 operand as two 16-bit pieces, three exact products, fp32 accumulate.  Tensors, parameters and results stay fp32.
The modes are entries of the library's option table (`SR_MLP_SPLIT`, `SR_WINO_SPLIT`: include/simplerecon_hip.h), set
through `_lib.set_option` -- the process environment is neither read nor written (r04 mutated os.environ, which the library
re-read with getenv() on every launch: a data race against launches on other threads, and inherited by child processes).
The SWITCH is process-wide: calls that OTHER threads start inside the block run split as well, and a HIP graph captured inside
the block keeps the split kernels after it.  A call in flight is not touched: each call reads its switch once and carries
that value from its weight packing to its launch (the Winograd format is an argument of both library calls and the key of
`ops.packed_wino_weight`'s cache; the sweep's entry point reads once).  The block must enclose the forward calls themselves."""
import contextlib

from . import _lib

_MODES = ("f16", "bf16")


@contextlib.contextmanager
def split_precision(mode="f16", sweep=True, convs=True):
    """mode: "f16" (as close to fp64 as the fp32 kernels on everything measured; operands must stay inside fp16's range,
    |x| < 65504, or the result is non-finite) or "bf16" (2-25 x coarser, fp32's range).  `sweep` / `convs` select the
    kernels.  Restores the previous switches on exit."""
    if mode not in _MODES:
        raise ValueError(f"split_precision mode must be one of {_MODES}, got {mode!r}")
    names = [n for n, on in (("SR_MLP_SPLIT", sweep), ("SR_WINO_SPLIT", convs)) if on]
    saved = {}
    try:
        for n in names:
            saved[n] = _lib.set_option(n, mode)
        yield
    finally:
        for n, v in saved.items():
            _lib.set_option(n, v)


@contextlib.contextmanager
def autocast_mfma16(mode=1, storage=True, wgrad=0):
    """16-bit MFMA convolutions for the training steps made inside the block, to be combined with torch.autocast:

        with torch.autocast("cuda", dtype=torch.bfloat16), experimental.autocast_mfma16():
            loss = model.step(...)

    Sets `autograd_ops.HALF_IO` (16-bit activations between the conv-stack layers), `autograd_ops.MFMA16 = mode` (1: the
    layers the measured rule sr_conv16_prefers accepts, 2: every layer sr_conv16_supported accepts) and, with `storage`,
    `autograd_ops.STORE_HALF` (saved activations in 16 bits) and `autograd_ops.MFMA16_WGRAD = wgrad` (0: weight / bias
    gradients and the activation derivative on fp32 copies, as before the switch existed; 1: the 16-bit weight gradient
    sr_conv16_wgrad_nhwc and the cast-free elementwise pass for the layers the rule sr_conv16_wgrad_prefers accepts, 2: for
    every layer sr_conv16_wgrad_supported accepts); restores the four previous values on exit.  The backward pass
    must run inside the block too (it reads the switches).  fp16, unlike bf16, needs a loss scaler.
    The switches are module attributes, hence process-wide: forward / backward passes that OTHER threads run while the block
    is open take the 16-bit paths as well."""
    from . import autograd_ops
    if mode not in (0, 1, 2):
        raise ValueError(f"autocast_mfma16 mode must be 0, 1 or 2, got {mode!r}")
    if wgrad not in (0, 1, 2):
        raise ValueError(f"autocast_mfma16 wgrad must be 0, 1 or 2, got {wgrad!r}")
    saved = (autograd_ops.HALF_IO, autograd_ops.MFMA16, autograd_ops.STORE_HALF, autograd_ops.MFMA16_WGRAD)
    try:
        autograd_ops.HALF_IO, autograd_ops.MFMA16, autograd_ops.MFMA16_WGRAD = True, mode, wgrad
        if storage:
            autograd_ops.STORE_HALF = True
        yield
    finally:
        autograd_ops.HALF_IO, autograd_ops.MFMA16, autograd_ops.STORE_HALF, autograd_ops.MFMA16_WGRAD = saved
