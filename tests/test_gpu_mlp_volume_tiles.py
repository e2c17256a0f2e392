"""Which 64 pixels form a wave of the metadata-MLP sweep (SR_MLP_TILE: the flattened strip, or 2x32 / 4x16 / 8x8 tiles)
changes which views a wave may skip as dead, and must change no bit of any result.  The cases build poses by hand so that
dead, live and mixed waves occur for tile-shaped waves (left / right tile columns, top / bottom tile rows, ragged tiles),
prove on the CPU (numpy fp64, the projection of csrc/sr_common.h, the lane -> pixel map of the shape the library reports)
that they do, and only then look at GPU output: every forced shape against SR_MLP_TILE=flat (torch.equal) and against the
CPU oracle (the bound of test_gpu_mlp_volume_dead_views.py)."""
import functools

import numpy as np
import pytest
import torch

import oracle
from parity import assert_close, mismatch_fraction
from simplerecon_amd import _lib, synthetic
from simplerecon_amd.cost_volume import FeatureVolumeManager, mlp_tile_shape, mlp_wave_pixels

DEV = "cuda:0"
B, C, D = 2, 16, 9            # D = 9: one full 8-plane unit and one partial one
PLANES = np.geomspace(0.25, 5.0, D)
MARGIN = 1e-3                 # texels between any sampling position and the edge of the region that has a tap
SHAPES = {"flat": (1, 64), "2x32": (2, 32), "4x16": (4, 16), "8x8": (8, 8)}
# (h, w, K)
MAPS = [
    (8, 32, 7),     # every shape exact
    (16, 8, 7),     # one 8x8 tile column
    (9, 17, 7),     # ragged in both directions for every 2-D shape: inactive rows and columns in one tile
    (10, 12, 7),    # no 2-D shape within 1 %: auto must answer flat
    (1, 70, 7),     # a single row: 2-D shapes are almost all padding
    (8, 32, 3),
    (9, 17, 3),
]
MAP_IDS = [f"{h}x{w}_k{k}" for h, w, k in MAPS]
# one string per batch element, one letter per view (_view)
VIEWS = {7: ("baltcab", "lbbtcbt"), 3: ("lat", "bcb")}


def _translation(tx, ty):
    T = np.eye(4)
    T[:3, 3] = (tx, ty, 0.0)
    return T


def _view(kind, f, h, w, i):
    """src_cam_T_cur_cam of one view.  With R = I and t = (tx, ty, 0) a plane at depth d samples at (x + f tx / d,
    y + f ty / d), and a pixel has a tap iff -1 < x + f tx / d < w and -1 < y + f ty / d < h.  `i` makes views of one
    kind differ a little."""
    e = 0.013 * i
    if kind == "a":   # near identity: every pixel has a tap at every plane (shift <= 0.8 texel at d = 0.25)
        return _translation((0.11 + e) / f, (-0.13 + e) / f)
    if kind == "b":   # large lateral offset: >= 6 w texels at the far plane: every pixel dead at every plane
        return _translation((30.3 * w + 7 * i) / f, 0.0)
    if kind == "c":   # to the right by 1.43 w texels at d = 1: dead at the near planes, the left part live at the far ones
        return _translation((1.43 * w + e) / f, 0.0)
    if kind == "l":   # to the left by w / 2 + 0.37 texels at plane 4: there the left half of the columns is dead
        return _translation(-(0.5 * w + 0.37 + e) * PLANES[4] / f, 0.0)
    if kind == "t":   # upwards by h / 2 + 0.37 texels at plane 4: there the top half of the rows is dead
        return _translation(0.0, -(0.5 * h + 0.37 + e) * PLANES[4] / f)
    raise KeyError(kind)


@functools.lru_cache(maxsize=None)
def _inputs(h, w, K):
    views = VIEWS[K]
    f = 0.625 * w
    Kmat = np.eye(4)
    Kmat[0, 0] = Kmat[1, 1] = f
    Kmat[0, 2], Kmat[1, 2] = w / 2.0, h / 2.0
    extr = np.stack([np.stack([_view(kind, f, h, w, i) for i, kind in enumerate(v)]) for v in views])
    rng = np.random.default_rng(500 + 10 * K + h)
    planes = np.broadcast_to(PLANES.astype(np.float32)[None, :, None, None], (B, D, h, w)).copy()
    return dict(
        cur_feats=torch.from_numpy(rng.standard_normal((B, C, h, w), dtype=np.float32)),
        src_feats=torch.from_numpy(rng.standard_normal((B, K, C, h, w), dtype=np.float32)),
        src_extrinsics=torch.from_numpy(extr.astype(np.float32)),
        src_poses=torch.from_numpy(np.linalg.inv(extr).astype(np.float32)),
        src_Ks=torch.from_numpy(np.broadcast_to(Kmat.astype(np.float32), (B, K, 4, 4)).copy()),
        cur_invK=torch.from_numpy(np.broadcast_to(np.linalg.inv(Kmat).astype(np.float32), (B, 4, 4)).copy()),
        min_depth=torch.tensor(synthetic.MIN_DEPTH).view(1, 1, 1, 1),
        max_depth=torch.tensor(synthetic.MAX_DEPTH).view(1, 1, 1, 1),
        depth_planes_bdhw=torch.from_numpy(planes),
    )


@functools.lru_cache(maxsize=None)
def _pixel_taps(h, w, K):
    """tap[b, k, j, pixel]: the pixel has a tap of view k inside the source image at plane j; and the smallest distance
    (texels) of any sampling position from the edge of the region that has one.  fp64 from the fp32 inputs, the steps of
    sr_project_sample_xy and sr_bilinear_taps: a tap is inside iff -1 <= ix < w and -1 <= iy < h."""
    n = {k: v.numpy().astype(np.float64) for k, v in _inputs(h, w, K).items()}
    N = h * w
    ys, xs = np.divmod(np.arange(N), w)
    pix = np.stack([xs + 0.5, ys + 0.5, np.ones(N)])
    tap = np.zeros((B, K, D, N), dtype=bool)
    margin = np.inf
    for b in range(B):
        rays = n["cur_invK"][b, :3, :3] @ pix
        for k in range(K):
            P = (n["src_Ks"][b, k] @ n["src_extrinsics"][b, k])[:3]
            for j in range(D):
                X = n["depth_planes_bdhw"][b, j].reshape(N) * rays
                q = P[:, :3] @ X + P[:, 3:4]
                zp = q[2] + 1e-8
                sc = np.where(np.abs(q[2]) > 1e-8, 1.0 / zp, 1.0)
                ix = ((2.0 * q[0] * sc / w - 1.0 + 1.0) * w - 1.0) / 2.0
                iy = ((2.0 * q[1] * sc / h - 1.0 + 1.0) * h - 1.0) / 2.0
                inside = np.minimum(np.minimum(ix + 1.0, w - ix), np.minimum(iy + 1.0, h - iy))
                tap[b, k, j] = inside > 0.0
                margin = min(margin, float(np.abs(inside).min()))
    return tap, margin


def wave_states(h, w, K, shape):
    """state[b, wave, plane, view]: 0 = no pixel of the wave has a tap (dead: what the kernel's ballot finds), 2 = every
    pixel has one, 1 = mixed, for waves of `shape` = (th, tw); ragged[wave]: the wave has lanes past the image, which do
    not vote."""
    tap, _ = _pixel_taps(h, w, K)
    lanes = mlp_wave_pixels(h, w, shape)                      # [waves, 64], -1 = inactive
    covered = np.sort(lanes[lanes >= 0])
    assert np.array_equal(covered, np.arange(h * w)), f"{shape} on {h}x{w}: the waves do not cover every pixel once"
    state = np.zeros((B, len(lanes), D, K), dtype=np.int64)
    for t, ln in enumerate(lanes):
        v = tap[..., ln[ln >= 0]]                             # [B, K, D, active lanes]
        state[:, t] = np.where(~v.any(-1), 0, np.where(v.all(-1), 2, 1)).transpose(0, 2, 1)
    return state, (lanes < 0).any(-1)


def check_patterns(h, w, K, shape):
    """What the cases were built for really occurs for waves of this shape, and robustly so in fp32."""
    name = f"{h}x{w} K={K} {shape[0]}x{shape[1]}"
    views = VIEWS[K]
    tap, margin = _pixel_taps(h, w, K)
    assert margin > MARGIN, f"{name}: a sampling position lies {margin:.2e} texel from the tap-validity boundary"
    img = tap.reshape(B, K, D, h, w)
    for b, v in enumerate(views):
        for k, kind in enumerate(v):
            t = img[b, k]
            if kind == "a":
                assert t.all(), f"{name}: view {k} of frame {b} is not live everywhere"
            if kind == "b":
                assert not t.any(), f"{name}: view {k} of frame {b} is not dead everywhere"
            if kind == "c":   # dead near, live far, inside the first 8-plane unit
                assert not t[0].any() and t[7].any(), f"{name}: view {k} of frame {b}: near / far"
            if kind == "l" and w > 1:   # at plane 4: dead columns left of live ones
                assert not t[4, :, :w // 2].any() and t[4, :, (w + 1) // 2:].all(), f"{name}: view {k} of frame {b}: left / right"
            if kind == "t" and h > 1:   # at plane 4: dead rows above live ones
                assert not t[4, :h // 2].any() and t[4, (h + 1) // 2:].all(), f"{name}: view {k} of frame {b}: top / bottom"
    state, ragged = wave_states(h, w, K, shape)
    dead = state == 0                                                     # [B, waves, D, K]
    assert dead.any() and (state == 2).any() and (state == 1).any(), f"{name}: dead / live / mixed waves"
    assert dead[..., 0].any(), f"{name}: dead view 0"
    assert dead[..., -1].any(), f"{name}: dead last view"
    assert (dead[..., 1:] & dead[..., :-1]).any(), f"{name}: two consecutive dead views"
    assert dead.all(-1).any(), f"{name}: all views dead"
    assert (~dead).any(-1).any(), f"{name}: no live view anywhere"
    if ragged.any():
        assert dead[:, ragged].any(), f"{name}: no dead view in a wave with inactive lanes"
    th, tw = shape
    if th > 1 and -(-h // th) > 1:   # a tile row above another: at one plane, a dead wave of the top row and a live one below
        tiles_x = -(-w // tw)
        top, bottom = dead[:, :tiles_x], ~dead[:, -tiles_x:]
        assert (top.any(1) & bottom.any(1)).any(), f"{name}: top tile row dead, bottom tile row live"
    if th > 1 and -(-w // tw) > 1:   # tile columns: at one plane, a dead wave of the left column and a live one of the right
        tiles_x = -(-w // tw)
        left, right = dead[:, 0::tiles_x], ~dead[:, tiles_x - 1::tiles_x]
        assert (left.any(1) & right.any(1)).any(), f"{name}: left tile column dead, right tile column live"
    if (h, w) == (9, 17) and th > 1:   # the cap: ragged tiles on both sides of the skip
        assert dead[:, ragged].any() and (~dead[:, ragged]).any(), f"{name}: dead and live waves with inactive lanes"
        assert ragged.sum() >= 2, f"{name}: ragged tiles"


def _forced_shape(h, w, name):
    """The (th, tw) the library reports for the map under SR_MLP_TILE=name."""
    prev = _lib.set_option("SR_MLP_TILE", name)
    try:
        return mlp_tile_shape(h, w)
    finally:
        _lib.set_option("SR_MLP_TILE", prev)


def test_chooser():
    """auto = the squarest 2-D shape whose tile count is at most 1 % above ceil(h w / 64), else the flattened strip; a forced
    shape is reported as forced; an unknown value is refused."""
    prev = _lib.set_option("SR_MLP_TILE", "auto")
    try:
        assert _lib.get_option("SR_MLP_TILE") == 0
        assert mlp_tile_shape(120, 160) == (8, 8) and mlp_tile_shape(96, 128) == (8, 8)
        assert mlp_tile_shape(180, 240) == (4, 16)
        assert mlp_tile_shape(10, 12) == (1, 64) and mlp_tile_shape(1, 70) == (1, 64)
        assert mlp_tile_shape(8, 32) == (8, 8) and mlp_tile_shape(16, 8) == (8, 8) and mlp_tile_shape(9, 17) == (1, 64)
        assert mlp_tile_shape(2, 64) == (2, 32) and mlp_tile_shape(4, 48) == (4, 16)
        rng = np.random.default_rng(5)
        sizes = [(int(h), int(w)) for h, w in rng.integers(1, 400, size=(300, 2))] + [(h, w) for h in range(1, 20) for w in range(1, 70)]
        for h, w in sizes:
            th, tw = mlp_tile_shape(h, w)
            flat = -(-h * w // 64)
            count = lambda t: -(-h // t) * -(-w // (64 // t))
            assert (th, tw) in SHAPES.values()
            if th > 1:
                assert 100 * count(th) <= 101 * flat, f"{h}x{w}: {th}x{tw} pads {count(th)} tiles against {flat}"
                assert all(100 * count(t) > 101 * flat for t in (8, 4, 2) if t > th), f"{h}x{w}: a squarer shape fits"
            else:
                assert all(100 * count(t) > 101 * flat for t in (8, 4, 2)), f"{h}x{w}: a 2-D shape fits"
            assert len(mlp_wave_pixels(h, w)) == (count(th) if th > 1 else flat)
        for name, shape in SHAPES.items():
            assert _forced_shape(9, 17, name) == shape and _forced_shape(120, 160, name) == shape
        _lib.set_option("SR_MLP_TILE", "16x4")                 # unknown
        with pytest.raises(_lib.HipLibraryError):
            mlp_tile_shape(120, 160)
    finally:
        _lib.set_option("SR_MLP_TILE", prev)
    with pytest.raises(_lib.HipLibraryError):
        mlp_tile_shape(0, 160)


@pytest.mark.parametrize("hwk", MAPS, ids=MAP_IDS)
def test_cases_hold_on_the_cpu(hwk):
    """The CPU half of the GPU tests below, for every forced shape (needs the library for the shape, not a GPU)."""
    for name in SHAPES:
        check_patterns(*hwk, _forced_shape(hwk[0], hwk[1], name))


@functools.lru_cache(maxsize=None)
def _manager(K, h, w):
    mgr = FeatureVolumeManager(h, w, num_depth_bins=D, matching_dim_size=C, num_source_views=K)
    synthetic.seeded_fill_(mgr.mlp, seed=60 + K)
    return mgr.to(DEV)


def _run(mgr, inp, tile, memory_format=torch.contiguous_format):
    """(volume, lowest-cost map, mask) under SR_MLP_TILE=tile."""
    prev = _lib.set_option("SR_MLP_TILE", tile)
    try:
        mgr.volume_memory_format = memory_format
        # the outputs are torch.empty: leave NaNs in the blocks the allocator is about to hand out again, so that a pixel no
        # wave owns does not inherit an earlier run's (correct) value
        b, _, h, w = inp["cur_feats"].shape
        d = inp["depth_planes_bdhw"].shape[1]
        poison = [torch.full((n,), float("nan"), device=DEV) for n in (b * d * h * w, b * h * w, b * h * w)]
        del poison
        with torch.inference_mode():
            vol, lowest, _, mask = mgr(return_mask=True, **{k: v.to(DEV) for k, v in inp.items()})
        torch.cuda.synchronize()
    finally:
        mgr.volume_memory_format = torch.contiguous_format
        _lib.set_option("SR_MLP_TILE", prev)
    return vol, lowest, mask


@functools.lru_cache(maxsize=None)
def _flat(h, w, K, channels_last):
    fmt = torch.channels_last if channels_last else torch.contiguous_format
    return _run(_manager(K, h, w), _inputs(h, w, K), "flat", fmt)


@functools.lru_cache(maxsize=None)
def _oracle(h, w, K):
    n = {k: v.numpy() for k, v in _inputs(h, w, K).items()}
    sd = {k: v.cpu().numpy() for k, v in _manager(K, h, w).mlp.state_dict().items()}
    mlp = dict(W1=sd["net.0.weight"], b1=sd["net.0.bias"], W2=sd["net.2.weight"], b2=sd["net.2.bias"],
               W3=sd["net.4.weight"], b3=sd["net.4.bias"])
    planes_np = np.broadcast_to(PLANES.astype(np.float32), (B, D)).copy()
    cv_o, _, mask_o = oracle.mlp_volume(n["cur_feats"], n["src_feats"], n["src_Ks"], n["src_extrinsics"], n["src_poses"],
                                        n["cur_invK"], planes_np, mlp, want_mask=True)
    return cv_o, mask_o


@pytest.mark.gpu
@pytest.mark.parametrize("hwk", MAPS, ids=MAP_IDS)
def test_mapping_changes_no_bit(hwk):
    """Volume, mask and lowest-cost map of every forced shape (and of auto) equal those of SR_MLP_TILE=flat, in both volume
    memory formats."""
    h, w, K = hwk
    for name in SHAPES:
        check_patterns(h, w, K, _forced_shape(h, w, name))               # before any GPU output is looked at
    for channels_last in (False, True):
        fmt = torch.channels_last if channels_last else torch.contiguous_format
        vol_f, lowest_f, mask_f = _flat(h, w, K, channels_last)
        for name in ("2x32", "4x16", "8x8", "auto"):
            vol, lowest, mask = _run(_manager(K, h, w), _inputs(h, w, K), name, fmt)
            what = f"{h}x{w} K={K} SR_MLP_TILE={name} {'channels-last' if channels_last else 'planar'}"
            assert vol.stride() == vol_f.stride(), what
            assert torch.equal(vol, vol_f), f"{what}: volume differs from flat"
            assert torch.equal(mask, mask_f), f"{what}: mask differs from flat"
            assert torch.equal(lowest, lowest_f), f"{what}: lowest-cost map differs from flat"


@pytest.mark.gpu
@pytest.mark.parametrize("hwk", MAPS, ids=MAP_IDS)
def test_every_shape_matches_oracle(hwk):
    """Each forced shape against the CPU oracle over the whole map (a pixel the ragged tiles miss or write twice shows
    here): the bound of the dead-view test, masks identical."""
    h, w, K = hwk
    for name in SHAPES:
        check_patterns(h, w, K, _forced_shape(h, w, name))               # before any GPU output is looked at
    cv_o, mask_o = _oracle(h, w, K)
    for name in SHAPES:
        vol, _, mask = _flat(h, w, K, False) if name == "flat" else _run(_manager(K, h, w), _inputs(h, w, K), name)
        assert_close(vol, cv_o, tol=2e-5, what=f"{h}x{w} K={K} SR_MLP_TILE={name} vs oracle")
        assert mismatch_fraction(mask, mask_o) == 0.0, f"{h}x{w} K={K} SR_MLP_TILE={name}: mask"


@pytest.mark.gpu
def test_vector_stores_of_ragged_tiles():
    """With a plane count that is a multiple of 4 the channels-last volume is written as 16-byte pieces per pixel at the end
    of a unit (the benchmark's path; D = 9 above takes the per-plane stores): ragged tiles of every shape store the flat
    strip's volume, and nothing outside it."""
    h, w, K, D8 = 9, 17, 3, 8
    inp = dict(_inputs(h, w, K))
    inp["depth_planes_bdhw"] = inp["depth_planes_bdhw"][:, :D8].contiguous()
    mgr = FeatureVolumeManager(h, w, num_depth_bins=D8, matching_dim_size=C, num_source_views=K)
    synthetic.seeded_fill_(mgr.mlp, seed=60 + K)
    mgr = mgr.to(DEV)
    planar = _run(mgr, inp, "flat")
    flat = _run(mgr, inp, "flat", torch.channels_last)
    assert flat[0].is_contiguous(memory_format=torch.channels_last) and torch.equal(flat[0].contiguous(), planar[0])
    for name in ("2x32", "4x16", "8x8"):
        got = _run(mgr, inp, name, torch.channels_last)
        for a, b, what in zip(got, flat, ("volume", "lowest-cost map", "mask")):
            assert torch.equal(a, b), f"SR_MLP_TILE={name}: {what} differs from flat"


@pytest.mark.gpu
def test_unknown_shape_is_refused_by_the_sweep():
    """An SR_MLP_TILE the library does not know launches nothing: the sweep fails loudly, and runs again once the option is back."""
    h, w, K = 8, 32, 3
    with pytest.raises(_lib.HipLibraryError):
        _run(_manager(K, h, w), _inputs(h, w, K), "16x4")
    assert torch.equal(_run(_manager(K, h, w), _inputs(h, w, K), "flat")[0], _flat(h, w, K, False)[0])
