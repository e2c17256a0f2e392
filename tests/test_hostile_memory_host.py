"""The hostile-memory helpers prove themselves on the CPU: the geometry of guarded views, and stand-in "kernels" written in
plain torch that commit each fault the GPU tests are after -- each one must be caught."""
import pytest
import torch
from torch import nn

import hostile_memory as hm
from hostile_memory import guarded, guard_damage, guard_intact, guard_mask, poisoned_empty
from simplerecon_amd import ops


def _image(shape, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype)


# ---- geometry ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape", [(1, 3, 5, 7), (2, 30, 4, 9), (3, 1, 2, 2), (2, 130, 1, 1), (2, 12, 3, 5)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_guarded_view_geometry_and_alignment(shape, offset, dtype):
    t = _image(shape, dtype)
    buffer, view = guarded(t, offset=offset)
    b, c, h, w = shape
    assert tuple(view.shape) == shape and view.dtype == dtype and torch.equal(hm.bits(view), hm.bits(t))
    assert ops._is_nhwc_view(view)
    assert view.untyped_storage().data_ptr() == buffer.untyped_storage().data_ptr()
    sb, sp = view.stride(0), view.stride(3)
    base = view.storage_offset() - buffer.storage_offset()
    assert sb % 4 == 0 and sp % 4 == 0 and base % 4 == offset
    # 16 BYTES in every dtype: 4 fp32 elements, 8 fp16 / bf16 ones -- base, pixel stride, row stride and image stride
    es = t.element_size()
    assert buffer.data_ptr() % 16 == 0 and (view.data_ptr() - buffer.data_ptr()) % 16 == offset * es
    assert all(view.stride(d) * es % 16 == 0 for d in (0, 2, 3))
    if dtype == torch.float32:
        assert bool(ops._aligned16(view, *ops._strides(view))) == (offset == 0)
    # guard bands on every side of the data: channels before and after each pixel, a gap between images, two pixel rows
    # at both ends
    assert sp >= c + 16 and sb >= h * w * sp + 64
    assert base >= 2 * w * sp and buffer.numel() - (base + (b - 1) * sb + h * w * sp) >= 2 * w * sp - 8
    mask = guard_mask(buffer, view)
    assert int((~mask).sum()) == t.numel()
    assert guard_damage(buffer, view) is None and guard_intact(buffer, view)
    assert bool(torch.isnan(buffer[mask]).all())


def test_guard_parameters_are_honoured():
    t = _image((2, 5, 3, 4))
    buffer, view = guarded(t, lead=4, tail=0, batch_gap=0, ends=8)
    assert view.stride(3) == 12 and view.stride(0) == 3 * 4 * 12 and view.storage_offset() == 8 + 4
    assert buffer.numel() == 16 + 2 * 144
    with pytest.raises(ValueError):
        guarded(t, lead=3)
    assert guarded(t, lead=3, offset=1)[1].storage_offset() % 4 == 0   # (3 + 1: the caller's business)


@pytest.mark.parametrize("offset", [0, 1])
def test_dense_form_keeps_the_layout_between_two_bands(offset):
    for t in (_image((7,)), _image((2, 3, 4)), _image((2, 5, 3, 4)).contiguous(memory_format=torch.channels_last),
              torch.arange(24, dtype=torch.int32).view(4, 6), torch.arange(12, dtype=torch.int64).view(3, 4).t()):
        buffer, view = guarded(t, dense=True, offset=offset)
        assert tuple(view.shape) == tuple(t.shape) and torch.equal(view, t)
        if hm._is_dense(t):
            assert view.stride() == t.stride()
        assert view.storage_offset() == 64 + offset and buffer.numel() == 128 + t.numel() + offset
        assert int((~guard_mask(buffer, view)).sum()) == t.numel()
        assert guard_intact(buffer, view)
        buffer[63 + offset] = 0
        assert guard_damage(buffer, view) == (63 + offset, (-1,))
        buffer, view = guarded(t, dense=True, offset=offset, ends=4)
        buffer[4 + offset + t.numel()] = 0
        assert guard_damage(buffer, view) == (4 + offset + t.numel(), (1,))
    assert not guarded(_image((2, 3, 4, 5)))[1].is_contiguous() and guarded(_image((2, 3, 4, 5)), dense=True)[1].is_contiguous()


def test_guard_damage_names_the_element():
    t = _image((2, 6, 3, 4))
    buffer, view = guarded(t)
    sb, _, sh, sp = view.stride()
    base = view.storage_offset()
    for rel, where in ((6, (0, 0, 0, 6)),                      # the channel behind the last one of pixel (0, 0)
                       (-1, (0, 0, 0, -1)),                    # the channel before the first one
                       (-sh, (0, -1, 0, 0)),                   # one row above image 0
                       (sb + 3 * sh, (1, 3, 0, 0)),            # one pixel past the last image
                       (3 * sh + 5, (0, 3, 0, 5)),             # the gap behind image 0
                       (sb + sh + 2 * sp + 7, (1, 1, 2, 7))):
        buffer2 = buffer.clone()
        view2 = buffer2.as_strided(view.shape, view.stride(), base)
        buffer2[base + rel] = 1.0
        assert guard_damage(buffer2, view2) == (base + rel, where)
        with pytest.raises(AssertionError, match="image, row, column, channel"):
            guard_intact(buffer2, view2)
    # a NaN of another payload is damage too: the check compares bits
    buffer[0] = float("nan")
    assert guard_damage(buffer, view)[0] == 0


# ---- stand-in kernels that commit each fault ---------------------------------------------------------------------------

def _conv1x1(x, weight, cin_read):
    """A 1x1 convolution that loads `cin_read` channels per pixel straight from memory and relies on zero-padded weights
    for the ones past Cin (cin_read == Cin: the honest kernel)."""
    b, c, h, w = x.shape
    wide = x.as_strided((b, cin_read, h, w), x.stride(), x.storage_offset())
    wpad = torch.zeros(weight.shape[0], cin_read)
    wpad[:, :c] = weight
    out = torch.zeros(b, weight.shape[0], h, w)
    for i in range(cin_read):   # one fixed summation order whatever the strides (a library contraction picks its own)
        out = out + wide[:, i:i + 1] * wpad[:, i].view(1, -1, 1, 1)
    return out


def test_read_one_channel_past_cin_times_a_zero_weight_is_caught():
    x, weight = _image((2, 5, 3, 4)), _image((7, 5), seed=1)
    want = _conv1x1(x, weight, 5)
    # on a dense tensor with a finite neighbour (the next pixel's first channel) the fault is invisible ...
    roomy = torch.cat([x.permute(0, 2, 3, 1).reshape(-1), torch.zeros(4)]).as_strided(x.shape, (60, 1, 20, 5))
    assert torch.equal(_conv1x1(roomy, weight, 6), want)
    # ... inside guard bands the honest kernel passes and the faulty one does not
    buffer, view = guarded(x)
    hm.assert_unaffected(want, _conv1x1(view, weight, 5), [(buffer, view)], [(view, x)])
    with pytest.raises(AssertionError, match="non-finite"):
        hm.assert_unaffected(want, _conv1x1(view, weight, 6), [(buffer, view)], [(view, x)])


def _column_sum3(x, from_memory):
    """out[y] = x[y-1] + x[y] + x[y+1] with zero padding; from_memory: the halo rows are loaded from the addresses above and
    below the image (what a kernel without a bounds check does)."""
    b, c, h, w = x.shape
    if from_memory:
        sb, sc, sh, sw = x.stride()
        halo = x.as_strided((b, c, h + 2, w), x.stride(), x.storage_offset() - sh)
    else:
        halo = torch.nn.functional.pad(x, (0, 0, 1, 1))
    return halo[:, :, :-2] + halo[:, :, 1:-1] + halo[:, :, 2:]


def test_read_one_row_above_image_0_is_caught():
    x = _image((1, 4, 3, 5))
    want = _column_sum3(x, False)
    zeros_around = torch.zeros(1, 4, 5, 5).contiguous(memory_format=torch.channels_last)
    zeros_around[:, :, 1:4] = x
    assert torch.equal(_column_sum3(zeros_around[:, :, 1:4], True), want)   # zero neighbours: exactly zero padding
    buffer, view = guarded(x)
    hm.assert_unaffected(want, _column_sum3(view, False), [(buffer, view)], [(view, x)])
    with pytest.raises(AssertionError, match="non-finite"):
        hm.assert_unaffected(want, _column_sum3(view, True), [(buffer, view)], [(view, x)])


def test_write_one_pixel_past_the_view_is_caught():
    x = _image((2, 4, 3, 5))
    buffer, out = guarded(torch.zeros_like(x))
    out.copy_(x * 2)
    hm.assert_unaffected(x * 2, out, [(buffer, out)])
    # the stand-in kernel rounds the pixel count of the last image up and stores one pixel too many
    sb, _, sh, sp = out.stride()
    past = out.storage_offset() + sb + 3 * sh
    buffer[past:past + 4] = 0.0
    with pytest.raises(AssertionError, match=r"\(1, 3, 0, 0\)"):
        hm.assert_unaffected(x * 2, out, [(buffer, out)])


@pytest.mark.parametrize("pattern", hm.PATTERNS)
def test_an_output_element_left_unwritten_is_caught(pattern):
    x = _image((1, 4, 3, 5)).abs()

    def kernel(x, skip):
        out = torch.empty_like(x)      # (the wrapper's allocation)
        flat, src = out.view(-1), (x * 2).view(-1)
        n = flat.numel() - (1 if skip else 0)
        flat[:n] = src[:n]
        return out
    want = x * 2
    with poisoned_empty(pattern):
        hm.assert_unaffected(want, kernel(x, False))
        bad = kernel(x, True)
    # 0xFF reads back as NaN; 0x7F as 3.39e38: finite, and only the comparison with the unpoisoned result sees it
    assert torch.isnan(bad.view(-1)[-1]) if pattern == 0xFF else float(bad.view(-1)[-1]) > 3e38
    with pytest.raises(AssertionError, match="non-finite" if pattern == 0xFF else "differ from the dense run"):
        hm.assert_unaffected(want, bad)
    # and a maximum over the unwritten element: 0xFF loses it (fmaxf and comparisons drop a NaN), 0x7F wins it
    fmax = float(torch.fmax(bad.view(-1), torch.zeros(())).max())
    assert (fmax == float(want.max())) == (pattern == 0xFF)


def test_a_modified_input_is_caught():
    x = _image((1, 4, 3, 5))
    buffer, view = guarded(x)
    view[0, 1, 2, 3] += 1.0
    with pytest.raises(AssertionError, match="input 0 was modified"):
        hm.assert_unaffected(x, x, [(buffer, view)], [(view, x)])


# ---- poisoned_empty --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pattern", hm.PATTERNS)
def test_poisoned_empty_fills_whole_storages_and_restores(pattern):
    real = (torch.empty, torch.empty_like)
    with poisoned_empty(pattern) as p:
        assert p == pattern and torch.empty is not real[0] and torch.empty_like is not real[1]
        f = torch.empty(3, 5)
        assert bool(torch.isnan(f).all()) if pattern == 0xFF else bool((f > 3e38).all() and torch.isfinite(f).all())
        assert bool(torch.isnan(torch.empty(4, dtype=torch.float16)).all())
        h = torch.empty(4, dtype=torch.bfloat16)     # 0x7F7F is a NaN in fp16 and 3.39e38 in bf16
        assert bool(torch.isnan(h).all()) if pattern == 0xFF else bool((h.float() > 3e38).all())
        i = torch.empty((2, 2), dtype=torch.int32)
        assert bool((i == (-1 if pattern == 0xFF else 0x7F7F7F7F)).all())
        like = torch.empty_like(torch.zeros(2, 3, 4, 5).contiguous(memory_format=torch.channels_last))
        assert like.is_contiguous(memory_format=torch.channels_last) and bool((hm.bits(like) == hm.bits(f)[0, 0]).all())
        assert torch.empty(3, dtype=torch.bool).dtype == torch.bool      # (left alone: any byte is a valid bool only as 0 / 1)
        assert torch.empty(3, device="meta").is_meta
        assert torch.empty(0).numel() == 0
        leaf = torch.empty(3, requires_grad=True)
        assert leaf.requires_grad and leaf.is_leaf
    assert (torch.empty, torch.empty_like) == real
    with pytest.raises(ValueError):
        with poisoned_empty(0x00):
            pass
    with pytest.raises(RuntimeError, match="boom"):
        with poisoned_empty(pattern):
            raise RuntimeError("boom")
    assert (torch.empty, torch.empty_like) == real


@pytest.mark.parametrize("pattern", hm.PATTERNS)
def test_torch_itself_stays_finite_under_the_patch(pattern):
    """Module construction, a forward pass and an optimiser step go through torch.empty in Python (parameter allocation) and
    initialise what they allocate: the patch must not break ordinary torch code around the kernels under test."""
    torch.manual_seed(0)
    with poisoned_empty(pattern):
        conv = nn.Conv2d(3, 4, 3, padding=1)
        opt = torch.optim.Adam(conv.parameters(), lr=1e-3)
        y = conv(torch.randn(2, 3, 5, 5))
        y.square().mean().backward()
        opt.step()
    assert bool(torch.isfinite(y).all()) and all(bool(torch.isfinite(p).all()) for p in conv.parameters())


def test_poison_fixture_runs_the_body_under_each_pattern(poison):
    from hostile_memory import PATTERNS
    assert poison in PATTERNS and int(hm.bits(torch.empty(1, dtype=torch.uint8))[0]) == poison


from hostile_memory import poison  # noqa: E402,F401  (the fixture, used by the test above)
