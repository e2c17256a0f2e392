"""Host side of the colour jitter (simplerecon_amd/frames.py jitter_params / JitterParams / train_tuple): ColorJitter's
range rules and draw sequence, the table the kernels read, and the oracle (tests/jitter_oracle.py) against the stored
fixture of tests/golden/make_jitter_golden.py.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import jitter_cases as jc
import jitter_oracle
from simplerecon_amd import _lib, frames
from simplerecon_amd._lib import HipLibraryError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_range_rules():
    r = frames.jitter_range
    assert r("brightness", 0.2) == (0.8, 1.2) and r("contrast", 0.5) == (0.5, 1.5)
    assert r("saturation", 1.5) == (0.0, 2.5)                       # max(0, 1 - a)
    assert r("hue", 0.2) == (-0.2, 0.2) and r("hue", 0.5) == (-0.5, 0.5)
    assert r("brightness", (0.3, 0.9)) == (0.3, 0.9) and r("hue", [-0.1, 0.3]) == (-0.1, 0.3)   # a pair as given
    # a range that collapses to the neutral value switches the operator off; any other single value does not
    assert r("brightness", 0) is None and r("hue", 0.0) is None and r("contrast", (1, 1)) is None and r("hue", (0, 0)) is None
    assert r("saturation", None) is None and r("contrast", (0.7, 0.7)) == (0.7, 0.7)
    for name, bad in (("brightness", -0.1), ("hue", 0.6), ("hue", (-0.6, 0.1)), ("contrast", (1.2, 0.8)),
                      ("saturation", (-0.1, 1.0))):
        with pytest.raises(ValueError):
            r(name, bad)
    with pytest.raises(TypeError):
        r("hue", (0.1, 0.2, 0.3))
    with pytest.raises(TypeError):
        r("hue", "0.1")
    with pytest.raises(ValueError):
        r("gamma", 0.1)
    with pytest.raises(ValueError):
        frames.FramePreparer(color_jitter=(0.2, 0.2, 0.2, 0.7))
    with pytest.raises(ValueError):
        frames.FramePreparer(color_jitter=(0.2, 0.2, 0.2))
    assert frames.FramePreparer().color_jitter is None
    assert frames.FramePreparer(color_jitter=[0.2, 0.2, 0.2, 0.2]).color_jitter == (0.2, 0.2, 0.2, 0.2)


@pytest.mark.parametrize("args", [(0.2, 0.2, 0.2, 0.2), (0.4, 0, (0.5, 1.5), 0), (0, 0, 0, 0), (0, 0.3, 0, (-0.5, 0.1))])
@pytest.mark.parametrize("use_generator", [False, True])
def test_draws_are_get_params_draws(args, use_generator):
    """Under one seed, jitter_params equals the calls ColorJitter.get_params makes, written out: an operator that is
    off draws nothing, so what follows it shifts forward in the stream."""
    ranges = [frames.jitter_range(n, v) for n, v in zip(frames.JITTER_OPS, args)]
    n = 5
    gen = torch.Generator().manual_seed(7) if use_generator else None
    if not use_generator:
        torch.manual_seed(7)
    want_order, want = [], []
    for _ in range(n):
        want_order.append(torch.randperm(4, generator=gen).tolist())
        want.append([float(torch.empty(1).uniform_(r[0], r[1], generator=gen)) if r is not None else neutral
                     for r, neutral in zip(ranges, (1.0, 1.0, 1.0, 0.0))])
    after = torch.rand(1, generator=gen).item()
    gen = torch.Generator().manual_seed(7) if use_generator else None
    if not use_generator:
        torch.manual_seed(7)
    p = frames.jitter_params(n, *args, generator=gen)
    assert torch.rand(1, generator=gen).item() == after            # the same number of draws was consumed
    assert p.order.dtype == np.int64 and p.order.tolist() == want_order
    assert p.factors.dtype == np.float64 and p.factors.tolist() == want
    assert p.on == tuple(r is not None for r in ranges) and len(p) == n
    for r, col in zip(ranges, p.factors.T):
        if r is not None:
            assert (col >= r[0]).all() and (col <= r[1]).all() and (col.astype(np.float32) == col).all()
    if use_generator:
        torch.manual_seed(123)
        state = torch.get_rng_state()
        frames.jitter_params(2, *args, generator=torch.Generator().manual_seed(1))
        assert torch.equal(torch.get_rng_state(), state)           # the global generator was left alone


def test_table_is_what_the_kernels_read():
    p = frames.JitterParams.from_values([[3, 1, 0, 2], [0, 1, 2, 3]], brightness=[0.5, 1.25], contrast=None,
                                        saturation=1.3, hue=[-0.5, 0.25])
    assert p.on == (True, False, True, True) and len(p) == 2
    t = p.table()
    assert t.dtype == np.int32 and t.shape == (2, frames.JITTER_WORDS) and t.flags.c_contiguous
    assert t[:, :4].tolist() == [[3, 0, 2, -1], [0, 2, 3, -1]]      # contrast is off: left out, the rest in order
    f = t[:, 4:].view(np.float32)
    assert f[:, 0].tolist() == [0.5, 1.25] and f[:, 1].tolist() == [0.5, -0.25]
    assert f[:, 2].tolist() == [1.0, 1.0] and f[:, 3].tolist() == [0.0, 0.0]          # an operator that is off: neutral
    # 1 - f in double, then rounded: not 1 - fp32(f)
    assert f[0, 4] == np.float32(1.3) and f[0, 5] == np.float32(1.0 - 1.3) != np.float32(1.0) - np.float32(1.3)
    assert f[:, 6].tolist() == [-0.5, 0.25] and (t[:, 11] == 0).all()
    none = frames.JitterParams.from_values([0, 1, 2, 3])
    assert len(none) == 1 and none.on == (False,) * 4 and none.table()[0, :4].tolist() == [-1] * 4
    for bad in ([0, 1, 2, 2], [0, 1, 2, 4], [0, 1, 2]):
        with pytest.raises(ValueError):
            frames.JitterParams.from_values(bad, 1.0, 1.0, 1.0, 0.0)
    with pytest.raises(ValueError):
        frames.JitterParams.from_values([0, 1, 2, 3], hue=0.6)
    with pytest.raises(ValueError):
        frames.JitterParams.from_values([0, 1, 2, 3], brightness=-0.1)
    with pytest.raises(ValueError):
        frames.JitterParams.from_values([0, 1, 2, 3], brightness=[1.0, 1.1], contrast=[1.0, 1.1, 1.2])
    with pytest.raises(ValueError):
        frames.jitter_params(0)


def test_train_tuple_draws_in_the_loaders_order(monkeypatch):
    """The flip once, then per frame randperm and one uniform_ per operator that is on -- the reference frame first.
    Counted by wrapping the three torch calls; FramePreparer.tuple is stubbed, so nothing is launched."""
    log = []
    rand, randperm, uniform_ = torch.rand, torch.randperm, torch.Tensor.uniform_

    def counted(name, fn):
        def wrapper(*a, **kw):
            log.append(name)
            return fn(*a, **kw)
        return wrapper
    monkeypatch.setattr(torch, "rand", counted("rand", rand))
    monkeypatch.setattr(torch, "randperm", counted("randperm", randperm))
    monkeypatch.setattr(torch.Tensor, "uniform_", counted("uniform_", uniform_))
    seen = {}

    def fake_tuple(self, frames_, flip=False, native_depth_size=None, jitter=None):
        seen.update(frames=frames_, flip=flip, jitter=jitter, size=native_depth_size)
        return "cur", "src"
    monkeypatch.setattr(frames.FramePreparer, "tuple", fake_tuple)
    tup = [("frame%d" % i,) for i in range(3)]

    prep = frames.FramePreparer(color_jitter=(0.2, 0.2, 0, 0.1))     # saturation off
    gen = torch.Generator().manual_seed(11)
    assert prep.train_tuple(tup, generator=gen, native_depth_size=(4, 5)) == ("cur", "src")
    assert log == ["rand"] + ["randperm", "uniform_", "uniform_", "uniform_"] * 3
    assert seen["frames"] == tup and seen["size"] == (4, 5)
    gen = torch.Generator().manual_seed(11)
    want_flip = rand(1, generator=gen).item() < 0.5
    want = frames.jitter_params(3, 0.2, 0.2, 0, 0.1, generator=gen)
    assert seen["flip"] is want_flip or seen["flip"] == want_flip
    assert seen["jitter"].order.tolist() == want.order.tolist() and seen["jitter"].factors.tolist() == want.factors.tolist()
    assert seen["jitter"].on == (True, True, False, True)
    assert (seen["jitter"].factors[:, 2] == 1.0).all()

    # the global generator serves when none is given; both flip outcomes occur over seeds
    flips = set()
    for seed in range(8):
        torch.manual_seed(seed)
        prep.train_tuple(tup)
        torch.manual_seed(seed)
        assert seen["flip"] == (rand(1).item() < 0.5)
        flips.add(bool(seen["flip"]))
    assert flips == {False, True}

    # without a colour transform only the flip is drawn
    del log[:]
    frames.FramePreparer().train_tuple(tup, generator=torch.Generator().manual_seed(1))
    assert log == ["rand"] and seen["jitter"] is None


def test_oracle_fp32_identity_for_neutral_factors():
    """f = 1 and 1 - f = 0: f x + 0 b is x exactly, so with hue off the chain returns to_tensor's image, whatever the
    order -- what lets the kernels promise prepare_color's bytes."""
    _, _, _, _, small = jc.case("ragged")
    x = jitter_oracle.to_tensor(small)
    for order in jc.ORDERS[::5]:
        order = np.tile(np.array(order), (3, 1))
        got = jitter_oracle.prepare(small, order, np.tile([1.0, 1.0, 1.0, 0.0], (3, 1)), (True, True, True, False),
                                    normalize=False)
        assert got.dtype == torch.float32 and torch.equal(got, x)
    cube = jc.cube_image()[None]
    got = jitter_oracle.prepare(cube, [[2, 1, 0, 3]], [[1.0, 1.0, 1.0, 0.0]], (True, True, True, False), normalize=False)
    assert torch.equal(got, jitter_oracle.to_tensor(cube))
    # and the normalised, flipped form is the loader's plain colour path
    import frames_oracle
    got = jitter_oracle.prepare(small, order, np.tile([1.0, 1.0, 1.0, 0.0], (3, 1)), (True, True, True, False), flip=True)
    want = frames_oracle.prepare_color(jc.case("ragged")[0], 37, 53, flip=True)
    assert got.numpy().tobytes() == np.ascontiguousarray(want).tobytes()


def test_oracle_pieces():
    """Spot values of the rule that need no package: greys keep their hue-shifted colour, a half turn of a primary is
    its complement, saturation 0 is the grey image, contrast 0 the mean grey."""
    grey = torch.full((3, 2, 2), 0.25, dtype=torch.float64)
    assert torch.equal(jitter_oracle.hue(grey, 0.3), grey)
    red = torch.tensor([1.0, 0.0, 0.0], dtype=torch.float64).view(3, 1, 1)
    assert torch.allclose(jitter_oracle.hue(red, 0.5), torch.tensor([0.0, 1.0, 1.0], dtype=torch.float64).view(3, 1, 1))
    assert torch.allclose(jitter_oracle.hue(red, -0.5), jitter_oracle.hue(red, 0.5))
    assert torch.allclose(jitter_oracle.hue(red, 1.0 / 3), torch.tensor([0.0, 1.0, 0.0], dtype=torch.float64).view(3, 1, 1),
                          atol=1e-15)
    img = jitter_oracle.to_tensor(jc.cube_image()[None], torch.float64)[0]
    assert torch.allclose(jitter_oracle.hue(img, 0.0), img, atol=1e-15)
    g = jitter_oracle.gray(img)
    assert torch.allclose(jitter_oracle.saturation(img, 0.0), g.expand(3, -1, -1))
    assert torch.allclose(jitter_oracle.contrast(img, 0.0), g.mean().expand(3, 64, 64))
    assert torch.equal(jitter_oracle.brightness(img, 2.0), (2 * img).clamp(0, 1))


@pytest.mark.parametrize("name", jc.GOLDEN_CASES)
def test_oracle_equals_stored_golden(name):
    gold = jc.load_golden()
    _, _, p, flip, small = jc.case(name)
    assert np.array_equal(gold[f"in_{name}"], small) and np.array_equal(gold[f"order_{name}"], p.order)
    assert np.array_equal(gold[f"factors_{name}"], p.factors) and tuple(gold[f"on_{name}"].tolist()) == p.on
    assert bool(gold[f"flip_{name}"]) == flip
    want = gold[f"f32_{name}"].astype(np.float64)
    assert want.shape == (small.shape[0], 3) + small.shape[1:3] and want.min() >= 0.0 and want.max() <= 1.0
    # the float64 oracle is what was stored (one fp32 rounding of a value in [0, 1], and the last bits of a mean)
    e64 = np.abs(jc.oracle(name, False, torch.float64).numpy() - want).max()
    assert e64 <= 2.0 ** -24, e64
    # and the fp32 oracle, torch's own roundings, lies within the bound the kernels are held to
    e32 = np.abs(jc.oracle(name, False, torch.float32).double().numpy() - want).max()
    assert 0 < e32 <= jc.bound(name) + 2.0 ** -25, (e32, jc.bound(name))
    assert jc.bound(name) < 1e-5 and jc.bound(name, True) < 5e-5     # a few fp32 roundings, nothing looser


def test_library_checks_the_table_and_the_sizes_on_the_host():
    hdr = open(os.path.join(ROOT, "include", "simplerecon_hip.h")).read()
    sec = hdr[hdr.index("Colour jitter:"):hdr.index("- visualisation -")]
    for phrase in ("UNPINNED", "0.2989 r + 0.587 g + 0.114 b", "randperm(4)", "no atomics", "18 bytes per pixel",
                   "#define SR_FRAMES_JITTER_PARAM_WORDS 12", "#define SR_FRAMES_JITTER_MAX_PARTIALS 128"):
        assert phrase in sec, phrase
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.lib()
    for name in ("sr_frames_jitter_scratch_bytes", "sr_frames_jitter_check_params", "sr_frames_jitter"):
        assert re.search(r"\b" + name + r"\s*\(", code) and name in _lib.SIGNATURES and hasattr(lib, name)
    good = frames.JitterParams.from_values([[3, 1, 0, 2], [0, 1, 2, 3]], 1.1, None, 0.9, 0.1).table()
    check = lambda t, n=2: lib.sr_frames_jitter_check_params(t.ctypes.data, n)
    assert check(good) == 0
    for slot, value in ((0, 4), (1, -2), (2, 3), (3, 7)):       # an unknown id; (2, 3): hue twice in frame 0
        bad = good.copy()
        bad[0, slot] = value
        assert check(bad) == 1, (slot, value)
    bad = good.copy()
    bad[1, 3] = bad[1, 0]                                       # the last frame is read too
    assert check(bad) == 1 and check(bad, 1) == 0
    assert lib.sr_frames_jitter_check_params(None, 2) == 1 and check(good, 0) == 1
    # sizes: refused before anything is launched (the pointers are never read)
    p = ctypes.c_void_p(1 << 20)
    run = lambda B, H, W, scratch=None, nbytes=0: lib.sr_frames_jitter(p, B, H, W, p, p, 0, 1, scratch, nbytes, None)
    assert run(1, frames.MAX_SIDE + 1, 4) == 2 and run(1, 4, frames.MAX_SIDE + 1) == 2 and run(frames.MAX_BATCH + 1, 4, 4) == 2
    assert run(0, 4, 4) == 2 and run(1, 0, 4) == 2
    assert lib.sr_frames_jitter(None, 1, 4, 4, p, p, 0, 1, None, 0, None) == 1
    assert lib.sr_frames_jitter(p, 1, 4, 4, ctypes.c_void_p((1 << 20) + 2), p, 0, 1, None, 0, None) == 1
    need = lib.sr_frames_jitter_scratch_bytes(3, 384, 512)
    assert need == 3 * 128 * 8 and lib.sr_frames_jitter_scratch_bytes(2, 37, 53) == 2 * 3 * 8
    assert lib.sr_frames_jitter_scratch_bytes(1, frames.MAX_SIDE + 1, 4) == 0
    assert run(3, 384, 512, p, need - 1) == 3                   # SR_ERR_WORKSPACE_TOO_SMALL
    assert run(3, 384, 512, ctypes.c_void_p((1 << 20) + 4), need) == 1


def test_no_gpu_means_an_error_not_a_fallback(monkeypatch):
    monkeypatch.setattr(frames._lib, "cuda_available", lambda: False)
    img = np.zeros((2, 8, 8, 3), dtype=np.uint8)
    p = frames.jitter_params(2, generator=torch.Generator().manual_seed(0))
    with pytest.raises(HipLibraryError):
        frames.prepare_color_jittered(img, 4, 4, p)
    with pytest.raises(TypeError):
        frames.prepare_color_jittered(img, 4, 4, "0.2")
    frame = (img[0], np.zeros((8, 8), dtype=np.uint16), np.eye(4), np.eye(4))
    prep = frames.FramePreparer(color_jitter=(0.2, 0.2, 0.2, 0.2))
    with pytest.raises(HipLibraryError):
        prep.frame(*frame, jitter=frames.JitterParams.from_values([0, 1, 2, 3], 1.1))
    with pytest.raises(HipLibraryError):
        prep.tuple([frame, frame], jitter=p)
    with pytest.raises(HipLibraryError):
        prep.train_tuple([frame, frame], generator=torch.Generator().manual_seed(0))
