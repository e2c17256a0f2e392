"""The case table of tests/tsdf_cases.py on the CPU: every case has the launch property it is listed for (tile form, tiles,
trips, partial tiles, LDS bytes, mesh bricks per scan thread), and -- from the numpy oracle alone -- none of them can pass
vacuously: every trip the plan has holds at least 5 % of the touched voxels, there are tiles with and without a touched
voxel, every fusion crop of the default volume has more than 1000 touched voxels (none behind the cameras), and the oracle
produces no NaN where the GPU comparison allows none (at most 1e-4 of the voxels elsewhere)."""
import numpy as np
import pytest

import oracle
import tsdf_cases as tc


# ------------------------------------------------------------------------------------------- plans ---------------
@pytest.mark.parametrize("dims, form, tiles, grid, trips, partial", [
    ((720, 728, 8), "small", 8190, 4096, 2, (0, 0, 8)),
    ((400, 408, 40), "small", 5100, 4096, 2, (0, 0, 8)),        # ntz = 2: the second z-tile holds 8 of 32 voxels
    ((1440, 1448, 8), "small", 32580, 4096, 8, (0, 0, 8)),      # 8190 large tiles: one short of the threshold
    ((1448, 1448, 8), "large", 8281, 4096, 3, (8, 8, 8)),
    ((504, 504, 504), "large", 8192, 4096, 2, (8, 8, 56)),      # OurFuser(): exactly on the threshold
    ((160, 160, 80), "small", 1200, 1200, 1, (0, 0, 16)),       # test_tsdf_full_size_properties: one trip
    ((64, 64, 64), "small", 128, 128, 1, (0, 0, 0)),
    ((32, 32, 32), "small", 16, 16, 1, (0, 0, 0)),
])
def test_tile_plan(dims, form, tiles, grid, trips, partial):
    p = tc.tile_plan(dims)
    assert (p["form"], p["tiles"], p["grid"], p["trips"], p["partial"]) == (form, tiles, grid, trips, partial)
    assert p["tile"] == (tc.LARGE_TILE if form == "large" else tc.SMALL_TILE)
    # the walk covers every voxel once: tile indices of all voxel columns are exactly 0 .. tiles - 1, trips 0 .. trips - 1
    ix, iy, iz = np.meshgrid(np.arange(0, dims[0], 8), np.arange(0, dims[1], 8), np.arange(0, dims[2], 8), indexing="ij")
    t = tc.tile_of(p, ix, iy, iz)
    assert np.array_equal(np.unique(t), np.arange(tiles))
    assert np.array_equal(np.unique(tc.trip_of(p, ix, iy, iz)), np.arange(trips))
    lin = np.ravel_multi_index((ix.ravel(), iy.ravel(), iz.ravel()), dims)
    t2, trip2 = tc.locate(p, dims, lin)
    assert np.array_equal(t2, t.ravel()) and np.array_equal(trip2, t.ravel() // grid)


def test_threshold_is_on_the_large_tile_count():
    assert tc.tile_plan((1440, 1448, 8))["large_tiles"] == 8190 and tc.tile_plan((1448, 1448, 8))["large_tiles"] == 8281
    assert tc.tile_plan((504, 504, 504))["large_tiles"] == tc.LARGE_FORM_TILES == 32 * 32 * 8
    assert 1440 * 1448 * 8 == 16_680_960 and 1448 * 1448 * 8 == 16_773_632
    # Z = 8 in a 64-deep tile: one active z-group (of the sub-brick's 4) in sub-brick 0, none in sub-brick 1
    assert tc.LARGE_TILE[2] // 32 == 2 and 8 // 8 == 1


def test_lds_bytes():
    assert tc.dynamic_lds_bytes(1024) == 50176 and tc.dynamic_lds_bytes(1024) <= 64 * 1024
    assert tc.dynamic_lds_bytes(5) == 256 and tc.dynamic_lds_bytes(300) == 48 * 300 + 16 * 19
    assert tc.BATCH_SIZES == (300, 1024, 1030) and tc.MAX_FRAMES == 1024


@pytest.mark.parametrize("dims, nbricks, chunk, busy", [
    ((64, 64, 64), 128, 1, 128),
    ((160, 160, 80), 1000, 1, 1000),
    ((160, 168, 128), 1680, 2, 840),
    ((200, 200, 160), 3125, 4, 782),          # threads >= 782 have no brick
    ((504, 504, 504), 62512, 62, 1009),       # 504 * 504 * 63 groups / 256
])
def test_mesh_plan(dims, nbricks, chunk, busy):
    p = tc.mesh_plan(dims)
    assert (p["nbricks"], p["chunk"], p["busy_threads"]) == (nbricks, chunk, busy)
    assert (busy - 1) * chunk < nbricks <= busy * chunk <= 1024 * chunk


def test_crop_coords_and_bounds():
    """Crop coordinates = the slice of the full grid the oracle generates; bounds_for gives back dims and origin."""
    origin, vs, dims = (8.4, -9.9, 7.7), 0.04, (24, 16, 40)
    o, d, coords, _, _ = oracle.tsdf_from_bounds(tc.bounds_for(origin, dims, vs), vs)
    assert d == dims and np.array_equal(o, np.asarray(origin, np.float32))
    lo, hi = (3, 0, 8), (20, 16, 24)
    crop = np.broadcast_to(tc.crop_coords(o, vs, lo, hi), (3, 17, 16, 16))
    assert np.array_equal(crop.view(np.uint16), coords[:, 3:20, 0:16, 8:24].view(np.uint16))
    for dims, vs in (((720, 728, 8), 0.02), ((1448, 1448, 8), 0.02), ((504, 504, 504), 0.04), ((400, 408, 40), 0.02)):
        b = tc.bounds_for((-1.0, 0.0, 1.0), dims, vs)
        assert tuple(int(np.ceil((b[a + "max"] - b[a + "min"]) / vs / 8)) * 8 for a in "xyz") == dims
    s = tc.default_volume_scene()
    assert s["bounds"]["xmin"] == -10.0 and np.array_equal(s["origin"], np.float32([-10, -10, -10]))


# ------------------------------------------------------------------------------------------- vacuity -------------
def _assert_not_vacuous(name, plan, index, nan_count):
    shares = tc.trip_shares(plan, index)
    print(f"{name}: {len(index[0])} touched, trip shares {np.round(shares, 3).tolist()}, "
          f"{len(tc.tiles_touched(plan, index))} of {plan['tiles']} tiles touched, {nan_count} NaN")
    assert len(shares) == plan["trips"] and shares.min() >= 0.05, f"{name}: trip shares {shares}"
    n = len(tc.tiles_touched(plan, index))
    assert 0 < n < plan["tiles"]
    assert nan_count == 0


@pytest.mark.parametrize("name", tc.SLAB_FULL)
def test_slab_full_cases(name):
    scene = tc.slab_case(name)
    plan = tc.tile_plan(scene["dims"])
    assert plan["form"] == "small" and plan["trips"] == 2
    v, w = tc.oracle_full(scene)
    _assert_not_vacuous(name, plan, tc.touched_index(v, w), int(np.isnan(v).sum()))
    assert not scene["mask"].all() and scene["mask"].all((1, 2, 3)).sum() == len(scene["mask"]) - 1


@pytest.mark.parametrize("name", tc.SLAB_CROPS)
def test_slab_crop_cases(name):
    scene = tc.slab_case(name)
    plan = tc.tile_plan(scene["dims"])
    assert (plan["form"], plan["trips"]) == (("large", 3) if name == "at_threshold_large" else ("small", 8))
    # no voxel is near a camera plane: the cull by pixel position is in force everywhere
    assert tc.slab_min_voxel_depth(scene) >= 1.0 > 0.25
    assert all(np.array_equal(T[:3, :3], np.eye(3)) and T[2, 3] == 0 for T in scene["T"])
    index, nan = [], 0
    for lo, hi, v, w in tc.slab_crops(name):
        assert not tc.crop_reaches_outer_layer(scene, lo, hi, v, w), f"{name}: crop {lo}..{hi} is too small"
        index.append(np.stack(tc.touched_index(v, w, lo)))
        nan += int(np.isnan(v).sum())
    # crops may overlap: count a voxel once
    index = np.unique(np.concatenate(index, 1), axis=1)
    _assert_not_vacuous(name, plan, tuple(index), nan)
    if plan["form"] == "large":   # the partial last tiles in x and in y are touched
        assert (index[0] >= 1440).any() and (index[1] >= 1440).any() and ((index[0] >= 1440) & (index[1] >= 1440)).any()


@pytest.mark.parametrize("name", list(tc.DEFAULT_CROPS))
def test_default_volume_crops(name):
    scene = tc.default_volume_scene()
    plan = tc.tile_plan(scene["dims"])
    assert plan["form"] == "large" and plan["trips"] == 2
    lo, hi = tc.DEFAULT_CROPS[name]
    shape = tuple(h - l for l, h in zip(lo, hi))
    assert np.prod(shape) <= 1_000_000 and shape[2] % 8 == 0
    v, w = tc.default_volume_crop(name)
    n = int(tc.touched_mask(v, w).sum())
    nan = int(np.isnan(v).sum())
    print(f"{name}: {n} touched of {v.size}, {nan} NaN")
    assert n == 0 if name == "behind" else n > 1000
    assert nan <= 1e-4 * v.size


def test_default_volume_crops_cover_both_trips_and_the_partial_tiles():
    scene = tc.default_volume_scene()
    plan = tc.tile_plan(scene["dims"])
    index = np.concatenate([np.stack(tc.touched_index(*tc.default_volume_crop(n), tc.DEFAULT_CROPS[n][0]))
                            for n in tc.DEFAULT_CROPS], 1)
    index = np.unique(index, axis=1)
    shares = tc.trip_shares(plan, tuple(index))
    print(f"default volume crops: trip shares {shares}")
    assert shares.min() >= 0.05
    assert (index[0] >= 496).any() and (index[1] >= 496).any()
    # the core crop straddles tile boundaries on every axis
    lo, hi = tc.DEFAULT_CROPS["core"]
    assert all(lo[a] // plan["tile"][a] < (hi[a] - 1) // plan["tile"][a] for a in range(3))


@pytest.mark.parametrize("which", list(tc.RANGE_ORIGINS))
def test_range_cases(which):
    scene = tc.range_scene(which)
    v, w = tc.oracle_full(scene)
    index = tc.touched_index(v, w)
    texel0 = int(tc.outside_every_frustum(scene, index).sum())
    nan = int(np.isnan(v).sum())
    print(f"range {which}: {len(index[0])} touched, {texel0} outside every frustum, {nan} NaN")
    assert len(index[0]) > 1000 and texel0 > 0
    assert nan <= 1e-4 * v.size
    if which == "far":   # every coordinate is past 4 in magnitude, most past 8: fp16 spacing 2^-8 .. 2^-7
        assert np.abs(scene["origin"]).min() > 7.5


def test_batch_cases():
    scene = tc.batch_scene()
    ref = tc.batch_oracle()
    assert sorted(ref) == [300, 1024, 1030]
    assert len(np.unique(scene["T"].reshape(len(scene["T"]), -1), axis=0)) == len(scene["T"])     # distinct poses
    assert 0.7 < scene["mask"].mean() < 0.9
    for B, (v, w) in ref.items():
        n = int(tc.touched_mask(v, w).sum())
        print(f"B = {B}: {n} touched, {int(np.isnan(v).sum())} NaN")
        assert n > 1000 and not np.isnan(v).any()
    # the frames past each smaller batch still change the volume: a dropped tail would be seen
    assert not np.array_equal(ref[300][0], ref[1024][0]) and not np.array_equal(ref[1024][0], ref[1030][0])
