"""Hostile memory around a kernel's logical operands.

The property the tests built on this module pin: a result depends only on the bytes of its logical inputs and parameters, and
a call writes only the bytes of its logical outputs.  Dense, freshly allocated test tensors hide violations of it (a halo load
past the image reads zero, a channel quad past Cin meets zero-padded weights, an element nobody writes reads back as the zero
it should have been), so:

* `poisoned_empty(pattern)` makes every `torch.empty` / `torch.empty_like` result arrive filled with one byte value;
* `guarded(t)` places a tensor inside a larger allocation whose every other element carries a fixed NaN bit pattern;
* `guard_intact(buffer, view)` checks bit for bit that those elements still do.

No GPU is needed to import or to use any of it."""
import contextlib

import pytest
import torch

# 0xFF: fp32 / fp16 / bf16 NaN, integers -1.  fmaxf, ordered comparisons and atomicMax swallow it (a NaN loses every
# comparison, -1 every signed maximum), so a maximum over unwritten memory still comes out right.
# 0x7F: fp32 and bf16 3.39e38 (finite), large positive integers, fp16 NaN.  It wins those maxima and survives a multiplication by
# zero, but a finite-ness check alone does not see it.  Each pattern catches what the other lets through.
PATTERNS = (0xFF, 0x7F)

# the guard value per element size: a quiet NaN with a recognisable payload in every floating-point format of that size
# (fp32 0x7FC5A5A5, fp16 0x7E5A, bf16 0x7FC5 -> as int16 below, fp64 0x7FF8...), a plain sentinel for integers
_GUARD_INT = {1: (torch.uint8, 0x5A), 2: (torch.int16, 0x7E5A), 4: (torch.int32, 0x7FC5A5A5),
              8: (torch.int64, 0x7FF8A5A5A5A5A5A5)}
_GUARD_BF16 = 0x7FC5


def _guard_word(dtype):
    idt, word = _GUARD_INT[torch.empty(0, dtype=dtype).element_size()]
    return idt, (_GUARD_BF16 if dtype == torch.bfloat16 else word)


def _quantum(dtype):
    """Elements per alignment unit: 16 bytes, and never fewer than 4 elements (4 for fp32, 8 for fp16 / bf16, 16 for bytes)."""
    return max(4, 16 // torch.empty(0, dtype=dtype).element_size())


def _up(n, q):
    return (n + q - 1) // q * q


# ---------------------------------------------------------------------------------------------------- poisoned_empty --

@contextlib.contextmanager
def poisoned_empty(pattern):
    """While active, every tensor `torch.empty` / `torch.empty_like` return has its WHOLE storage filled with the byte
    `pattern` (one of PATTERNS).  bool and meta tensors are left alone.  Both functions are restored on exit, exception or
    not."""
    if pattern not in PATTERNS:
        raise ValueError(f"pattern must be one of {[hex(p) for p in PATTERNS]}, got {pattern!r}")
    real_empty, real_empty_like = torch.empty, torch.empty_like

    def poison(t):
        if not isinstance(t, torch.Tensor) or t.dtype == torch.bool or t.is_meta or t.layout != torch.strided:
            return t
        storage = t.untyped_storage()
        nbytes = storage.nbytes()
        if nbytes:
            with torch.no_grad():
                real_empty(0, dtype=torch.uint8, device=t.device).set_(storage, 0, (nbytes,), (1,)).fill_(pattern)
        return t

    def empty(*args, **kwargs):
        return poison(real_empty(*args, **kwargs))

    def empty_like(*args, **kwargs):
        return poison(real_empty_like(*args, **kwargs))

    torch.empty, torch.empty_like = empty, empty_like
    try:
        yield pattern
    finally:
        torch.empty, torch.empty_like = real_empty, real_empty_like


@pytest.fixture(params=PATTERNS, ids=[f"poison_{p:#04x}" for p in PATTERNS])
def poison(request):
    """The test body runs under `poisoned_empty`, once per pattern (import the fixture into the test module)."""
    with poisoned_empty(request.param) as pattern:
        yield pattern


# ----------------------------------------------------------------------------------------------------------- guarded --

def guarded(t, *, lead=8, tail=8, batch_gap=64, ends=None, offset=0, dense=None):
    """(buffer, view): `view` has `t`'s shape and values and sits inside the one larger allocation `buffer`, whose every
    other element carries the guard NaN of `t`'s dtype.

    A 4-D `t` (dense=None / False) becomes a channels-last view that `ops._is_nhwc_view` accepts: `lead` and `tail` guard
    channels inside each pixel stride, `batch_gap` guard elements between images, `ends` (default: two pixel rows of the
    guarded layout, at least 64) before the first and after the last image.  With offset=0 the base address and both strides
    are multiples of 16 bytes and of 4 elements (4 fp32 elements, 8 fp16 / bf16 ones), so a dispatcher picks the kernel it
    picks for a dense tensor (`lead` must then be such a multiple; the pixel stride, the gap and `ends` are rounded up to
    one); offset=1 shifts the view by one element: the misaligned variant, for the scalar paths.

    Any other `t`, or dense=True (a wrapper that cannot take a strided view), keeps `t`'s own dense layout between two
    `ends` bands (default 64 elements)."""
    if dense is None:
        dense = t.dim() != 4
    idt, word = _guard_word(t.dtype)
    q = _quantum(t.dtype)
    if dense:
        ends = _up(64 if ends is None else ends, q)
        flat = t.contiguous() if not _is_dense(t) else t
        span = flat.numel()
        buffer = torch.empty(2 * ends + span + offset, dtype=t.dtype, device=t.device)
        buffer.view(idt).fill_(word)
        view = buffer.as_strided(flat.shape, flat.stride(), ends + offset)
        view.copy_(flat)
        return buffer, view
    if lead % q and offset == 0:
        raise ValueError(f"lead must be a multiple of {q} elements (16 bytes) for the aligned variant")
    b, c, h, w = t.shape
    pix = _up(lead + c + tail, q)
    img = h * w * pix + _up(batch_gap, q)
    ends = _up(max(2 * w * pix, 64) if ends is None else ends, q)
    buffer = torch.empty(2 * ends + b * img + offset, dtype=t.dtype, device=t.device)
    buffer.view(idt).fill_(word)
    view = buffer.as_strided((b, c, h, w), (img, 1, w * pix, pix), ends + lead + offset)
    view.copy_(t)
    return buffer, view


def _is_dense(t):
    """Non-overlapping and without holes: the strides are those of a contiguous tensor in some dimension order."""
    expect = 1
    for size, stride in sorted(((s, st) for s, st in zip(t.shape, t.stride()) if s != 1), key=lambda p: p[1]):
        if stride != expect:
            return False
        expect *= size
    return True


def guard_mask(buffer, view):
    """bool tensor over `buffer`: True on guard elements, False on the elements of `view`."""
    mask = torch.ones(buffer.numel(), dtype=torch.bool, device=buffer.device)
    mask.as_strided(view.shape, view.stride(), view.storage_offset() - buffer.storage_offset()).fill_(False)
    return mask


def guard_damage(buffer, view):
    """None while every guard element of `buffer` still holds its bit pattern (compared as integers), else the first damaged
    one as (flat offset in the buffer, (image, row, column, channel) relative to `view`) -- coordinates past the view's
    extent or below zero say on which side it lies; for a dense-form view the tuple is (elements before the view's start
    or past its end,)."""
    idt, word = _guard_word(buffer.dtype)
    bad = (buffer.view(idt) != word) & guard_mask(buffer, view)
    hits = torch.nonzero(bad)
    if hits.numel() == 0:
        return None
    at = int(hits[0])
    rel = at - (view.storage_offset() - buffer.storage_offset())
    if view.dim() == 4 and view.stride(1) == 1 and not _is_dense(view):
        b, c, h, w = view.shape
        img, _, row_stride, pix = view.stride()
        if b == 1:
            img = h * row_stride
        image = min(max(rel // img, 0), b - 1)
        rem = rel - image * img
        row = rem // row_stride
        rem -= row * row_stride
        col, ch = rem // pix, rem % pix
        if ch >= c + (pix - c) // 2:   # nearer the next pixel's first channel: its lead band
            col, ch = col + 1, ch - pix
            if col == w:
                row, col = row + 1, 0
        return at, (image, row, col, ch)
    return at, (rel if rel < 0 else rel - view.numel() + 1,)


def guard_intact(buffer, view, what="buffer"):
    """True, or an AssertionError that names the first damaged guard element."""
    damage = guard_damage(buffer, view)
    if damage is not None:
        at, where = damage
        names = "(image, row, column, channel)" if len(where) == 4 else "(offset from the view)"
        raise AssertionError(f"{what}: guard element {at} was overwritten, at {names} = {where} relative to the view")
    return True


def bits(t):
    """`t`'s elements as integers of the same size, in a dense tensor (what 'bitwise equal' compares)."""
    idt, _ = _guard_word(t.dtype)
    return t.contiguous().view(idt)


def assert_unaffected(plain, got, guards=(), inputs=(), what="result"):
    """The checks every guarded run ends with: `got` (a tensor or a sequence of them) is finite wherever it is floating point
    and bit-equal to `plain` (the same op on dense operands), every (buffer, view) of `guards` is intact, and every (view,
    original) of `inputs` still holds the original's bits."""
    plains, gots = (plain, got) if isinstance(plain, (list, tuple)) else ((plain,), (got,))
    assert len(plains) == len(gots)
    for i, (p, g) in enumerate(zip(plains, gots)):
        if p is None and g is None:
            continue
        assert tuple(p.shape) == tuple(g.shape) and p.dtype == g.dtype, (what, i, p.shape, g.shape)
        if g.is_floating_point():
            finite = torch.isfinite(g)
            assert bool(finite.all()), \
                f"{what}[{i}]: {int((~finite).sum())} non-finite elements, first at {tuple(torch.nonzero(~finite)[0].tolist())}"
        same = bits(p) == bits(g)
        assert bool(same.all()), \
            f"{what}[{i}]: {int((~same).sum())} elements differ from the dense run, first at {tuple(torch.nonzero(~same)[0].tolist())}"
    for i, (buffer, view) in enumerate(guards):
        guard_intact(buffer, view, what=f"{what}: guarded operand {i}")
    for i, (view, original) in enumerate(inputs):
        assert torch.equal(bits(view), bits(original)), f"{what}: input {i} was modified"
