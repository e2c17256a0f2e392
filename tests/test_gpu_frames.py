"""Frame preparation on the GPU (simplerecon_amd/frames.py, csrc/sr_frames.hip) against the fixtures Pillow and
torch's CPU kernels wrote (tests/golden/make_frames_golden.py).  Every comparison is exact: equal bytes, NaNs in
equal places.  There is no tolerance in this feature."""
import numpy as np
import pytest
import torch
from torch.utils.data import default_collate

import frames_cases as fc
import frames_oracle
from simplerecon_amd import depth_model as dm
from simplerecon_amd import frames
from simplerecon_amd._lib import HipLibraryError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def color():
    return fc.load("color")


@pytest.fixture(scope="module")
def depth():
    return fc.load("depth")


@pytest.fixture(scope="module")
def tup():
    return fc.load("tuple")


def _same_bits(got, want):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    return got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()


def _paths(fn):
    """(result, path) of one colour call: which of the two kernels paths ran, from the module's counters."""
    before = dict(frames.path_counts)
    out = fn()
    ran = [k for k in before if frames.path_counts[k] != before[k]]
    assert len(ran) == 1 and frames.path_counts[ran[0]] == before[ran[0]] + 1
    return out, ran[0]


@pytest.mark.parametrize("name", sorted(fc.COLOR_CASES))
def test_resize_and_prepare_color_equal_pillow(color, name):
    B, h, w, C, H, W = fc.COLOR_CASES[name]
    img = torch.from_numpy(color[f"in_{name}"]).to(DEV)
    got, path = _paths(lambda: frames.resize_u8(img, H, W))
    assert path == ("two_pass" if name == "steep" else "fused")
    assert got.dtype == torch.uint8 and got.device == img.device
    assert _same_bits(got, color[f"u8_{name}"])
    if C == 3:
        got, path = _paths(lambda: frames.prepare_color(img, H, W))
        assert path == ("two_pass" if name == "steep" else "fused")
        assert _same_bits(got, color[f"f32_{name}"])
    if name in fc.FLIP_CASES:
        assert _same_bits(frames.prepare_color(img, H, W, flip=True), color[f"f32flip_{name}"])


def test_both_paths_give_the_same_bytes(color, monkeypatch):
    """The two-launch path on shapes the fused kernel serves, by declaring that nothing fits LDS."""
    class NoLds:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            return (lambda *a: 0) if name == "sr_frames_resize_fits_lds" else getattr(self._lib, name)
    real = frames._lib.lib()
    monkeypatch.setattr(frames._lib, "lib", lambda: NoLds(real))
    for name in ("wide", "up", "tiles", "four"):
        H, W = fc.COLOR_CASES[name][4:]
        img = torch.from_numpy(color[f"in_{name}"]).to(DEV)
        got, path = _paths(lambda: frames.resize_u8(img, H, W))
        assert path == "two_pass" and _same_bits(got, color[f"u8_{name}"])
    got, path = _paths(lambda: frames.prepare_color(torch.from_numpy(color["in_wide"]).to(DEV), 48, 67, flip=True))
    assert path == "two_pass" and _same_bits(got, color["f32flip_wide"])


@pytest.mark.parametrize("name", fc.FILTER_CASES)
@pytest.mark.parametrize("resample", fc.OTHER_FILTERS)
def test_other_filters_equal_pillow(color, resample, name):
    H, W = fc.COLOR_CASES[name][4:]
    got = frames.resize_u8(torch.from_numpy(color[f"in_{name}"]).to(DEV), H, W, resample)
    assert _same_bits(got, color[f"u8_{resample}_{name}"])


def test_production_shape_against_the_oracle():
    """One ScanNet-sized frame, 968 x 1296 -> 384 x 512 with flip: every tile position of the real workload.  The
    oracle is pinned to Pillow by tests/test_frames_host.py."""
    img = np.random.default_rng(3).integers(0, 256, (1, 968, 1296, 3), dtype=np.uint8)
    got, path = _paths(lambda: frames.prepare_color(torch.from_numpy(img).to(DEV), 384, 512, flip=True))
    assert path == "fused"
    assert _same_bits(got, frames_oracle.prepare_color(img, 384, 512, flip=True))


def test_offsets_past_two_gib():
    """Three images of 805 MB: the last one starts past 2^31 bytes and must come out as when resized on its own."""
    g = torch.Generator(device=DEV).manual_seed(5)
    img = torch.randint(0, 256, (3, 32768, 8192, 3), dtype=torch.uint8, device=DEV, generator=g)
    assert img.numel() > 2 ** 31
    got, path = _paths(lambda: frames.resize_u8(img, 16384, 4096))
    assert path == "fused"
    alone = frames.resize_u8(img[2:3].clone(), 16384, 4096)
    assert torch.equal(got[2:3], alone) and not torch.equal(got[0], got[2])
    rows = frames_oracle.resize_u8(img[2:3, -40:, -64:].cpu().numpy(), 20, 32)     # the last corner, on the host
    assert _same_bits(got[2:3, -12:, -20:], rows[:, -12:, -20:])


@pytest.mark.parametrize("dtype", [torch.uint16, torch.int32])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("name", sorted(fc.DEPTH_CASES))
def test_prepare_depth_equals_torch_cpu(depth, name, flip, dtype):
    H, W = fc.DEPTH_CASES[name][2:]
    d = torch.from_numpy(depth[f"in_{name}"].astype(np.int32)).to(dtype).to(DEV) if dtype == torch.int32 else \
        torch.from_numpy(depth[f"in_{name}"]).to(DEV)
    got = frames.prepare_depth(d, H, W, flip=flip)
    tag = "flip_" if flip else ""
    assert [g.dtype for g in got] == [torch.float32, torch.float32, torch.bool]
    for g, key in zip(got, ("depth", "mask", "mask_b")):
        assert _same_bits(g, depth[f"{key}_{tag}{name}"]), key
    assert torch.isnan(got[0]).any() and torch.equal(torch.isnan(got[0]), ~got[2])


def _tuple_frames(tup, on_device):
    conv = (lambda a: torch.from_numpy(a).to(DEV)) if on_device else (lambda a: a)
    return [(conv(tup["colors"][i]), conv(tup["depths"][i]), tup["world_T_cam"][i], tup["K"], f"frame-{i:04d}")
            for i in range(4)]


@pytest.mark.parametrize("flip", [False, True])
def test_tuple_equals_fixture_key_by_key(tup, flip):
    prep = frames.FramePreparer(**fc.TUPLE)
    cur, src = prep.tuple(_tuple_frames(tup, on_device=not flip), flip=flip)
    tag = "flip" if flip else "plain"
    order = tup[f"{tag}_order"].tolist()
    want_keys = {k[len(tag) + 5:] for k in tup if k.startswith(f"{tag}_cur_")} | {"image_b3hw", "high_res_color_b3hw"}
    assert set(cur) == set(src) == want_keys | {"frame_id_string"}
    assert cur["frame_id_string"] == "frame-0000" and src["frame_id_string"] == [f"frame-{1 + i:04d}" for i in order]
    for k in sorted(want_keys):
        want_cur, want_src = tup.get(f"{tag}_cur_{k}"), tup.get(f"{tag}_src_{k}")
        if want_cur is None:      # the flipped colour images: the plain fixture mirrored, sources in this order
            want_cur = tup[f"plain_cur_{k}"][..., ::-1]
            plain = dict(zip(tup["plain_order"].tolist(), tup[f"plain_src_{k}"]))
            want_src = np.stack([plain[i] for i in order])[..., ::-1]
        assert cur[k].is_cuda and src[k].is_cuda
        assert _same_bits(cur[k], want_cur), k
        assert _same_bits(src[k], want_src), k
    assert cur["image_b3hw"].shape == (3, 96, 128) and src["image_b3hw"].shape == (3, 3, 96, 128)
    assert cur["full_res_depth_b1hw"].shape == (1, 48, 64) and src["mask_b_b1hw"].dtype == torch.bool
    one = prep.frame(*_tuple_frames(tup, True)[0][:4], flip=flip)
    assert "frame_id_string" not in one
    assert all(_same_bits(one[k], cur[k].cpu().numpy()) for k in one)
    # get_frame's load_depth=False: no depth keys, the intrinsics scaled from the size the caller names
    plain = frames.FramePreparer(**dict(fc.TUPLE, include_full_res_depth=False))
    color_only = plain.frame(tup["colors"][0], None, tup["world_T_cam"][0], tup["K"], flip=flip, native_depth_size=(48, 64))
    assert set(color_only) == {k for k in cur if "depth" not in k and "mask" not in k and k != "frame_id_string"} | {
        "K_full_depth_b44", "invK_full_depth_b44"}
    assert all(_same_bits(color_only[k], cur[k].cpu().numpy()) for k in color_only)
    with pytest.raises(ValueError):
        plain.frame(tup["colors"][0], None, tup["world_T_cam"][0], tup["K"])


def test_prepared_tuple_runs_through_depth_model(tup):
    H, W, K = 96, 128, 2
    prep = frames.FramePreparer(image_height=H, image_width=W, depth_height=H // 2, depth_width=W // 2)
    cur, src = default_collate([prep.tuple(_tuple_frames(tup, True)[: K + 1])])
    model = dm.DepthModel(dm.default_options(image_width=W, image_height=H, model_num_views=K + 1,
                                             matching_num_depth_bins=8)).to(DEV).eval()
    with torch.inference_mode():
        out = model("test", cur, src, unbatched_matching_encoder_forward=True, return_mask=True)
    pred = out["depth_pred_s0_b1hw"]
    assert pred.shape == (1, 1, H // 2, W // 2) and torch.isfinite(pred).all()


def test_repeatable_and_stream_independent(color, depth):
    img = torch.from_numpy(color["in_tiles"]).to(DEV)
    d = torch.from_numpy(depth["in_down"]).to(DEV)
    first = [frames.prepare_color(img, 35, 150, flip=True), frames.resize_u8(img, 35, 150, "lanczos"),
             *frames.prepare_depth(d, 19, 25)]
    again = [frames.prepare_color(img, 35, 150, flip=True), frames.resize_u8(img, 35, 150, "lanczos"),
             *frames.prepare_depth(d, 19, 25)]
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        other = [frames.prepare_color(img, 35, 150, flip=True), frames.resize_u8(img, 35, 150, "lanczos"),
                 *frames.prepare_depth(d, 19, 25)]
    side.synchronize()
    for a, b, c in zip(first, again, other):
        assert _same_bits(a, b.cpu().numpy()) and _same_bits(a, c.cpu().numpy())


def test_errors(color, monkeypatch):
    img = torch.from_numpy(color["in_ragged"]).to(DEV)
    with pytest.raises(TypeError):
        frames.resize_u8(img.float(), 11, 17)
    with pytest.raises(TypeError):
        frames.prepare_depth(torch.zeros(1, 8, 8, device=DEV), 4, 4)
    with pytest.raises(ValueError):
        frames.resize_u8(torch.zeros(1, 8, 8, 5, dtype=torch.uint8, device=DEV), 4, 4)
    with pytest.raises(ValueError):
        frames.prepare_color(torch.zeros(1, 8, 8, 4, dtype=torch.uint8, device=DEV), 4, 4)
    with pytest.raises(ValueError):
        frames.resize_u8(img, 0, 17)
    with pytest.raises(ValueError):
        frames.prepare_depth(torch.zeros(1, 8, 8, dtype=torch.int32, device=DEV), 4, 0)
    with pytest.raises(ValueError):
        frames.resize_u8(img[0], 11, 17)
    with pytest.raises(ValueError):
        frames.resize_u8(img, 11, 17, "nearest")
    # host data is a convenience copy while a GPU is visible, an error when none is: never a CPU computation
    assert _same_bits(frames.resize_u8(color["in_ragged"], 11, 17), color["u8_ragged"])
    monkeypatch.setattr(frames._lib, "cuda_available", lambda: False)
    with pytest.raises(HipLibraryError):
        frames.resize_u8(img.cpu(), 11, 17)
