"""Host side of frame preparation (simplerecon_amd/frames.py): the Pillow coefficient and nearest-index tables, the
intrinsics pyramid and the source ordering, against fixtures written by tests/golden/make_frames_golden.py with
Pillow and torch's CPU kernels.  tests/frames_oracle.py (numpy, driven by those tables) is what the GPU tests compare
the kernels with, so it is pinned to Pillow here.  No GPU."""
import numpy as np
import pytest
import torch

import frames_cases as fc
import frames_oracle
from simplerecon_amd import frames
from simplerecon_amd._lib import HipLibraryError
from simplerecon_amd.keyframes import sort_sources_by_pose_penalty


@pytest.fixture(scope="module")
def color():
    return fc.load("color")


@pytest.fixture(scope="module")
def depth():
    return fc.load("depth")


@pytest.fixture(scope="module")
def tup():
    return fc.load("tuple")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", sorted(fc.COLOR_CASES))
def test_oracle_resize_equals_pillow_fixture(color, name):
    B, h, w, C, H, W = fc.COLOR_CASES[name]
    img = color[f"in_{name}"]
    assert img.shape == (B, h, w, C)
    assert name == "pixel" or {0, 255} <= set(np.unique(img).tolist())     # the clamps and the rounding are hit
    assert _same_bits(frames_oracle.resize_u8(img, H, W), color[f"u8_{name}"])
    if C == 3:
        assert _same_bits(frames_oracle.prepare_color(img, H, W), color[f"f32_{name}"])
    if name in fc.FLIP_CASES:
        assert _same_bits(frames_oracle.prepare_color(img, H, W, flip=True), color[f"f32flip_{name}"])


@pytest.mark.parametrize("name", fc.FILTER_CASES)
@pytest.mark.parametrize("resample", fc.OTHER_FILTERS)
def test_oracle_other_filters_equal_pillow_fixture(color, resample, name):
    H, W = fc.COLOR_CASES[name][4:]
    got = frames_oracle.resize_u8(color[f"in_{name}"], H, W, resample)
    assert _same_bits(got, color[f"u8_{resample}_{name}"])
    assert got.min() == 0 and got.max() == 255       # the 0 / 255 edges reach both clamps


@pytest.mark.parametrize("name", sorted(fc.DEPTH_CASES))
@pytest.mark.parametrize("flip", [False, True])
def test_oracle_depth_equals_torch_fixture(depth, name, flip):
    H, W = fc.DEPTH_CASES[name][2:]
    d = depth[f"in_{name}"]
    assert set(fc.DEPTH_SPECIALS) <= set(np.unique(d).tolist())
    tag = "flip_" if flip else ""
    for dt in (np.uint16, np.int32):
        got = frames_oracle.prepare_depth(d.astype(dt), H, W, flip=flip)
        for g, key in zip(got, ("depth", "mask", "mask_b")):
            assert _same_bits(g, depth[f"{key}_{tag}{name}"]), key
    # the boundaries, as torch's CPU comparison placed them: 1 mm and 10 000 mm are invalid, 2 mm and 9 999 mm valid
    if name == "same" and not flip:
        ok = depth["mask_b_same"][:, 0]
        for mm, valid in ((0, False), (1, False), (2, True), (9999, True), (10000, False), (10001, False), (65535, False)):
            assert (ok[d == mm] == valid).all(), mm


def test_oracle_equals_pillow_on_random_shapes():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(11)
    for i in range(12):
        h, w, H, W = (int(v) for v in rng.integers(1, 90, 4))
        resample = ("bilinear", "bicubic", "lanczos", "box", "hamming")[i % 5]
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(img, "RGB").resize((W, H), resample=getattr(Image, resample.upper())))
        assert _same_bits(frames_oracle.resize_u8(img[None], H, W, resample)[0], ref), (h, w, H, W, resample)
        d = rng.integers(0, 65536, (h, w)).astype(np.uint16)
        ref = np.asarray(Image.fromarray(d).resize((W, H), resample=Image.NEAREST))
        got = d[frames.nearest_table(h, H)][:, frames.nearest_table(w, W)]
        assert _same_bits(got, ref), (h, w, H, W)


def test_tables():
    first, count, weights = frames.resample_tables(968, 384)
    assert first.dtype == count.dtype == weights.dtype == np.int32 and weights.shape == (384, int(count.max()))
    assert (first >= 0).all() and (first + count <= 968).all() and (count >= 1).all()
    assert (np.abs(weights.sum(1) - (1 << 22)) <= count).all()          # each row sums to one, up to its roundings
    assert frames.rows_needed(first, count) == max(
        (first[y:y + 16] + count[y:y + 16]).max() - first[y] for y in range(0, 384, 16))
    first, count, weights = frames.resample_tables(64, 64, "lanczos")   # a skipped pass: the identity
    assert (first == np.arange(64)).all() and (count == 1).all() and (weights == 1 << 22).all()
    assert frames.nearest_table(4, 10).tolist() == [0, 0, 1, 1, 1, 2, 2, 3, 3, 3]
    assert frames.nearest_table(7, 7).tolist() == list(range(7))
    with pytest.raises(ValueError):
        frames.resample_tables(10, 5, "nearest")
    with pytest.raises(ValueError):
        frames.resample_tables(10, 0)
    with pytest.raises(ValueError):
        frames.nearest_table(0, 3)


@pytest.mark.parametrize("flip", [False, True])
def test_scaled_intrinsics_equal_fixture(tup, flip):
    tag = "flip" if flip else "plain"
    got = frames.scaled_intrinsics(tup["K"], 64, 48, fc.TUPLE["depth_width"], fc.TUPLE["depth_height"], flip=flip,
                                   include_full_depth_K=True)
    names = [f"{p}K_s{i}_b44" for i in range(5) for p in ("", "inv")] + ["K_full_depth_b44", "invK_full_depth_b44"]
    assert sorted(got) == sorted(names)
    for n in names:
        assert got[n].dtype == torch.float32 and _same_bits(got[n].numpy(), tup[f"{tag}_cur_{n}"]), n
    assert "K_full_depth_b44" not in frames.scaled_intrinsics(tup["K"], 64, 48, 32, 24)
    assert tup["flip_cur_K_s0_b44"][0, 2] != tup["plain_cur_K_s0_b44"][0, 2]


@pytest.mark.parametrize("flip", [False, True])
def test_source_order_and_poses_equal_fixture(tup, flip):
    tag = "flip" if flip else "plain"
    pairs = [frames.flipped_pose(p, flip) for p in tup["world_T_cam"]]
    assert _same_bits(pairs[0][0], tup[f"{tag}_cur_world_T_cam_b44"])
    assert _same_bits(pairs[0][1], tup[f"{tag}_cur_cam_T_world_b44"])
    order = sort_sources_by_pose_penalty(pairs[0][1], np.stack([p[0] for p in pairs[1:]]))
    assert order == tup[f"{tag}_order"].tolist() and order != sorted(order)
    assert _same_bits(np.stack([pairs[1 + i][0] for i in order]), tup[f"{tag}_src_world_T_cam_b44"])


def test_normalise_table_is_torchs_rounding(color):
    lut = frames.normalise_table()
    assert lut.shape == (3, 256) and lut.dtype == torch.float32
    u8, ref = color["u8_wide"], color["f32_wide"]
    assert _same_bits(np.stack([lut[c].numpy()[u8[..., c]] for c in range(3)], axis=1), ref)


def test_no_gpu_means_an_error_not_a_fallback(monkeypatch):
    monkeypatch.setattr(frames._lib, "cuda_available", lambda: False)
    img = np.zeros((1, 8, 8, 3), dtype=np.uint8)
    with pytest.raises(HipLibraryError):
        frames.resize_u8(img, 4, 4)
    with pytest.raises(HipLibraryError):
        frames.prepare_depth(np.zeros((1, 8, 8), dtype=np.uint16), 4, 4)
    with pytest.raises(HipLibraryError):
        frames.FramePreparer().frame(img[0], np.zeros((8, 8), dtype=np.uint16), np.eye(4), np.eye(4))
