"""The colour jitter on the GPU (simplerecon_amd/frames.py prepare_color_jittered, csrc/sr_frames_jitter.hip) against
tests/jitter_oracle.py, the rule in torch's CPU operations (parity against the torchvision package itself is unpinned:
it is absent here).

Tolerance, per case, measured on the case's own inputs on the CPU (tests/jitter_cases.py bound): with
e32 = max |oracle_fp32 - oracle_fp64|, the un-normalised GPU result lies within max(4 e32, 2^-22) of the float64
oracle; normalised, within that / 0.224 + 2^-21.  No pixel is left out.  Where no operator changes a value the result
is prepare_color's, byte for byte, and two runs always give equal bytes.

Measured errors of a run are written to $SR_JITTER_PARITY_OUT (json) when that variable is set
(profiles/jitter_parity.json)."""
import json
import os

import numpy as np
import pytest
import torch

import jitter_cases as jc
from simplerecon_amd import frames

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    path = os.environ.get("SR_JITTER_PARITY_OUT")
    if path and RECORD:
        with open(path, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "reference": "tests/jitter_oracle.py in float64",
                       "bound": "max(4 e32, 2^-22); normalised: / 0.224 + 2^-21", "cases": RECORD}, f, indent=1)
            f.write("\n")


def _same_bits(a, b):
    a, b = a.contiguous().cpu().numpy(), b.contiguous().cpu().numpy()
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _check(name, normalize=False):
    img, (H, W), p, flip, _ = jc.case(name)
    got = frames.prepare_color_jittered(torch.from_numpy(img).to(DEV), H, W, p, flip=flip, normalize=normalize)
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == (img.shape[0], 3, H, W)
    got = got.cpu()
    assert torch.isfinite(got).all()
    err = float((got.double() - jc.oracle(name, normalize, torch.float64)).abs().max())
    vs32 = float((got - jc.oracle(name, normalize, torch.float32)).abs().max())
    bound = jc.bound(name, normalize)
    RECORD[name + ("_normalised" if normalize else "")] = {"e32": jc.e32(name), "gpu_error": err, "bound": bound,
                                                           "gpu_vs_oracle_fp32": vs32, "pixels": int(got[:, 0].numel())}
    print(f"{name} normalize={normalize}: e32 {jc.e32(name):.3g} gpu_error {err:.3g} bound {bound:.3g} vs fp32 {vs32:.3g}")
    assert err <= bound, (name, normalize, err, bound)
    if not normalize:
        assert got.min() >= 0.0 and got.max() <= 1.0
    return got


def test_cube_every_operator_order():
    """The 16^3 lattice -- greys, primaries, black, white, every tie of the largest channel -- under all 24 orders,
    one per frame, factors from the default ranges."""
    _, _, p, _, _ = jc.case("cube")
    assert sorted(map(tuple, p.order.tolist())) == sorted(jc.ORDERS) and all(p.on)
    got = _check("cube")
    assert len({got[i].numpy().tobytes() for i in range(24)}) == 24     # the frame's own parameters reached it
    _check("cube", normalize=True)


def test_edges_of_the_ranges_and_beyond():
    _, _, p, _, _ = jc.case("edges")
    assert [tuple(f) for f in p.factors.tolist()[::2]] == list(jc.EDGE_FACTORS)
    assert p.order.tolist()[:2] == [list(jc.CONTRAST_FIRST), list(jc.CONTRAST_LAST)]
    _check("edges")


@pytest.mark.parametrize("normalize", [False, True])
def test_ragged_rows_with_flip(normalize):
    """W % 4 = 1: the byte path, rows that start in the middle of a wave, a last lane with one pixel."""
    _, (H, W), _, flip, _ = jc.case("ragged")
    assert W % 4 == 1 and flip
    _check("ragged", normalize)


def test_several_groups_and_determinism():
    """Many workgroup partials per frame, contrast after hue; and the same bytes on a second run."""
    _, _, p, _, _ = jc.case("several_groups")
    assert p.order.tolist() == [list(jc.CONTRAST_AFTER_HUE)]
    first = _check("several_groups")
    again = _check("several_groups")
    assert _same_bits(first, again)
    _check("several_groups", normalize=True)


def test_strided_mean_pass():
    """More workgroups than partials: the mean pass strides over the frame; flipped wide stores."""
    _, (H, W), _, flip, _ = jc.case("strided")
    assert W % 4 == 0 and flip and (W // 4 * H + 255) // 256 > 128
    first = _check("strided")
    assert _same_bits(first, _check("strided"))


@pytest.mark.parametrize("on", jc.OFF_SUBSETS, ids=lambda on: "".join("01"[v] for v in on))
def test_operators_switched_off(on):
    name = "off_" + "".join("01"[v] for v in on)
    assert jc.case(name)[2].on == on
    _check(name, normalize=not on[0])


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("name", ["ragged", "wide"])
def test_exact_where_nothing_changes(name, flip):
    """All operators off, and factors (1, 1, 1) with hue off, return prepare_color's bytes."""
    img = jc.case("ragged")[0] if name == "ragged" else jc.noise(11, 2, 70, 300)
    H, W = (37, 53) if name == "ragged" else (35, 152)            # wider than 128 columns
    img = torch.from_numpy(img).to(DEV)
    B = img.shape[0]
    want = frames.prepare_color(img, H, W, flip=flip)
    off = frames.JitterParams.from_values(np.tile([2, 0, 3, 1], (B, 1)))
    assert _same_bits(frames.prepare_color_jittered(img, H, W, off, flip=flip), want)
    for order in ([0, 1, 2, 3], [1, 2, 0, 3], [2, 3, 1, 0]):
        ones = frames.JitterParams.from_values(np.tile(order, (B, 1)), 1.0, 1.0, 1.0, None)
        assert _same_bits(frames.prepare_color_jittered(img, H, W, ones, flip=flip), want), order
    raw = frames.prepare_color_jittered(img, H, W, off, flip=flip, normalize=False)
    small = frames.resize_u8(img, H, W).cpu().permute(0, 3, 1, 2).float().div(255)      # to_tensor, on the CPU as the loader
    assert _same_bits(raw, torch.flip(small, (-1,)) if flip else small)


def test_resample_and_argument_errors():
    img, (H, W), p, flip, _ = jc.case("ragged")
    dev = torch.from_numpy(img).to(DEV)
    got = frames.prepare_color_jittered(dev, H, W, p, resample="bicubic", flip=flip, normalize=False)
    import frames_oracle
    import jitter_oracle
    small = frames_oracle.resize_u8(img, H, W, "bicubic")
    want = jitter_oracle.prepare(small, p.order, p.factors, p.on, flip=flip, normalize=False, dtype=torch.float64)
    assert float((got.cpu().double() - want).abs().max()) <= jc.bound("ragged")
    with pytest.raises(ValueError):
        frames.prepare_color_jittered(dev[:2], H, W, p)                 # three frames of parameters for two images
    with pytest.raises(TypeError):
        frames.prepare_color_jittered(dev, H, W, None)
    with pytest.raises(ValueError):
        frames.prepare_color_jittered(dev[..., :1], H, W, p)


def _tuple_frames(on_device):
    import frames_cases as fc
    tup = fc.load("tuple")
    conv = (lambda a: torch.from_numpy(a).to(DEV)) if on_device else (lambda a: a)
    return fc, tup, [(conv(tup["colors"][i]), conv(tup["depths"][i]), tup["world_T_cam"][i], tup["K"], f"frame-{i:04d}")
                     for i in range(4)]


@pytest.mark.parametrize("flip", [False, True])
def test_frame_preparer_tuple_with_jitter(flip):
    fc, tup, fr = _tuple_frames(on_device=True)
    prep = frames.FramePreparer(**fc.TUPLE)
    p = frames.jitter_params(4, generator=torch.Generator().manual_seed(5))
    cur0, src0 = prep.tuple(fr, flip=flip)
    cur, src = prep.tuple(fr, flip=flip, jitter=p)
    images = frames.prepare_color_jittered(torch.from_numpy(tup["colors"]).to(DEV), fc.TUPLE["image_height"],
                                           fc.TUPLE["image_width"], p, flip=flip)
    order = tup["flip_order" if flip else "plain_order"].tolist()
    assert _same_bits(cur["image_b3hw"], images[0])
    assert _same_bits(src["image_b3hw"], torch.stack([images[1 + i] for i in order]))
    assert not torch.equal(cur["image_b3hw"], cur0["image_b3hw"])
    assert set(cur) == set(cur0) and set(src) == set(src0) and "high_res_color_b3hw" in cur
    for k in cur0:          # nothing but image_b3hw changes: high_res_color_b3hw and every depth key included
        if k == "frame_id_string":
            assert cur[k] == cur0[k] and src[k] == src0[k]
        elif k != "image_b3hw":
            assert _same_bits(cur[k], cur0[k]) and _same_bits(src[k], src0[k]), k
    one = prep.frame(*fr[0][:4], flip=flip, jitter=frames.JitterParams(p.order[:1], p.factors[:1], p.on))
    assert _same_bits(one["image_b3hw"], images[0]) and _same_bits(one["depth_b1hw"], cur0["depth_b1hw"])
    with pytest.raises(ValueError):
        prep.tuple(fr[:3], flip=flip, jitter=p)
    with pytest.raises(TypeError):
        prep.tuple(fr, flip=flip, jitter=(0.2, 0.2, 0.2, 0.2))


def test_train_tuple_under_a_seed():
    """train_tuple equals tuple with the flip and the parameters drawn by hand in the loader's order; over seeds both
    flip outcomes occur."""
    fc, tup, fr = _tuple_frames(on_device=False)
    prep = frames.FramePreparer(color_jitter=jc.DEFAULT, **fc.TUPLE)
    flips = set()
    for seed in (0, 1, 2, 3):
        cur, src = prep.train_tuple(fr, generator=torch.Generator().manual_seed(seed))
        gen = torch.Generator().manual_seed(seed)
        flip = torch.rand(1, generator=gen).item() < 0.5
        order, factors = [], []
        for _ in range(4):
            order.append(torch.randperm(4, generator=gen).tolist())
            factors.append([float(torch.empty(1).uniform_(lo, hi, generator=gen))
                            for lo, hi in ((0.8, 1.2), (0.8, 1.2), (0.8, 1.2), (-0.2, 0.2))])
        by_hand = frames.JitterParams(order, factors, (True,) * 4)
        want_cur, want_src = prep.tuple(fr, flip=flip, jitter=by_hand)
        for k in want_cur:
            if k == "frame_id_string":
                assert cur[k] == want_cur[k] and src[k] == want_src[k]
            else:
                assert _same_bits(cur[k], want_cur[k]) and _same_bits(src[k], want_src[k]), k
        flips.add(flip)
        if len(flips) == 2:
            break
    assert flips == {False, True}
    torch.manual_seed(9)
    a = prep.train_tuple(fr)[0]["image_b3hw"]
    torch.manual_seed(9)
    assert _same_bits(a, prep.train_tuple(fr)[0]["image_b3hw"])       # the global generator serves by default


def test_captures_in_a_graph():
    """Both launches record into a HIP graph: the call allocates nothing the graph does not own and never waits for
    the host.  The replay gives the eager bytes."""
    img, (H, W), p, flip, _ = jc.case("several_groups")
    dev = torch.from_numpy(img).to(DEV)
    eager = frames.prepare_color_jittered(dev, H, W, p, flip=flip)
    small = frames.resize_u8(dev, H, W)
    table = torch.from_numpy(p.table()).to(DEV)
    nbytes = int(frames._lib.lib().sr_frames_jitter_scratch_bytes(1, H, W))
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=DEV)
    out = torch.zeros((1, 3, H, W), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        frames._lib.call("sr_frames_jitter", out.device, small, 1, H, W, table, out, int(flip), 1, scratch, nbytes)
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(out, eager)
