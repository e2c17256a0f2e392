"""The dense fuser (csrc/sr_tsdf.hip) by value where its launch changes form (cases and plan arithmetic: tests/tsdf_cases.py,
checked on the CPU by tests/test_tsdf_cases_host.py): a workgroup's second and later tiles, both sides of the threshold
between the 8 x 8 x 32 and the 16 x 16 x 64 tile, the default 504^3 volume with 640 x 480 frames at f = 577.87, the production
numeric range on a small volume, and batches of 300, 1024 and 1030 frames.  Values and weights are compared BIT FOR BIT with
the numpy oracle (uint16 views; positions that are NaN on both sides are left out and counted)."""
import numpy as np
import pytest
import torch

import tsdf_cases as tc
from simplerecon_amd import _lib
from simplerecon_amd.tsdf import TSDF, OurFuser, TSDFFuser

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _half(scene, key, frames=slice(None)):
    return None if scene[key] is None else torch.from_numpy(scene[key][frames]).to(DEV).half()


def _mask(scene, frames=slice(None)):
    return None if scene["mask"] is None else torch.from_numpy(scene["mask"][frames]).to(DEV)


def _fuse(scene, vol=None):
    """The scene's frames in one integrate_depth call into a generated-coordinate volume over the scene's bounds."""
    if vol is None:
        vol = TSDF.from_bounds(dict(scene["bounds"]), scene["voxel_size"], device=DEV)
    assert tuple(vol.tsdf_values.shape) == scene["dims"]
    if vol._generated:
        assert np.array_equal(vol._origin_f32.numpy(), scene["origin"])
    fuser = TSDFFuser(vol, min_depth=scene["min_depth"], max_depth=scene["max_depth"])
    fuser.integrate_depth(_half(scene, "depth"), _half(scene, "T"), _half(scene, "K"), depth_mask_b1hw=_mask(scene))
    return vol


def _assert_equal(scene, got_v, got_w, want_v, want_w, lo=(0, 0, 0), nan_cap=0.0, what=""):
    """Bit-for-bit equality of a (crop of a) volume with its reference; a mismatch is reported with its tile and trip."""
    gv = got_v.cpu().numpy() if isinstance(got_v, torch.Tensor) else got_v
    gw = got_w.cpu().numpy() if isinstance(got_w, torch.Tensor) else got_w
    assert gv.shape == want_v.shape
    bad = (gv.view(np.uint16) != want_v.view(np.uint16)) | (gw.view(np.uint16) != want_w.view(np.uint16))
    nan_both = np.isnan(gv) & np.isnan(want_v)
    excluded = int(nan_both.sum())
    assert excluded <= nan_cap * gv.size, f"{what}: {excluded} of {gv.size} voxels are NaN on both sides"
    bad &= ~nan_both
    if bad.any():
        plan = tc.tile_plan(scene["dims"])
        ix, iy, iz = (i + l for i, l in zip(np.nonzero(bad), lo))
        tiles = tc.tile_of(plan, ix, iy, iz)
        pytest.fail(f"{scene['name']} {what}: {int(bad.sum())} voxels differ of {int(tc.touched_mask(want_v, want_w).sum())} "
                    f"touched ({plan['form']} tiles); first at {(int(ix[0]), int(iy[0]), int(iz[0]))}: tile {int(tiles[0])}, "
                    f"trip {int(tiles[0]) // plan['grid']}; trips hit {np.unique(tiles // plan['grid']).tolist()}, "
                    f"{len(np.unique(tiles))} tiles")


def _crop(t, lo, hi):
    return t[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]]


# ------------------------------------------------------------------------------------------- 2a ------------------
@pytest.mark.parametrize("name", tc.SLAB_FULL)
def test_second_trip_small_tiles(name):
    """8190 and 5100 tiles of 8 x 8 x 32 on 4096 workgroups: a workgroup's second tile reuses the frame flags and the kept-frame
    counter in LDS.  Three frames (one behind a mask) against the oracle on the whole volume; no NaN anywhere."""
    scene = tc.slab_case(name)
    plan = tc.tile_plan(scene["dims"])
    assert plan["form"] == "small" and plan["trips"] == 2
    vol = _fuse(scene)
    v, w = tc.oracle_full(scene)
    assert tc.trip_shares(plan, tc.touched_index(v, w)).min() >= 0.05
    _assert_equal(scene, vol.tsdf_values, vol.tsdf_weights, v, w, what="whole volume")


# ------------------------------------------------------------------------------------------- 2b ------------------
@pytest.mark.parametrize("name", tc.SLAB_CROPS)
def test_tile_form_threshold(name):
    """The two smallest volumes around the form threshold (16.7 M voxels each): 8190 large tiles -> 32 580 small tiles in 8
    trips; 8281 large tiles -> the 16 x 16 x 64 form in 3 trips, Z = 8 leaving one z-group of sub-brick 0 active and sub-brick 1
    empty.  Reference: the oracle on one crop per camera (the crops are checked on the CPU to hold everything the oracle
    touches), and (-1, 0) everywhere outside the crops."""
    scene = tc.slab_case(name)
    plan = tc.tile_plan(scene["dims"])
    assert plan["form"] == ("large" if name == "at_threshold_large" else "small")
    assert tc.slab_min_voxel_depth(scene) >= 1.0      # no voxel near a camera plane: culling by pixel position everywhere
    vol = _fuse(scene)
    outside = torch.ones(scene["dims"], dtype=torch.bool, device=DEV)
    index = []
    for lo, hi, v, w in tc.slab_crops(name):
        assert not tc.crop_reaches_outer_layer(scene, lo, hi, v, w)
        _assert_equal(scene, _crop(vol.tsdf_values, lo, hi), _crop(vol.tsdf_weights, lo, hi), v, w, lo=lo,
                      what=f"crop {lo}..{hi}")
        _crop(outside, lo, hi).fill_(False)
        index.append(np.stack(tc.touched_index(v, w, lo)))
    assert tc.trip_shares(plan, tuple(np.unique(np.concatenate(index, 1), axis=1))).min() >= 0.05
    stray = outside & ((vol.tsdf_values != -1) | (vol.tsdf_weights != 0))
    if bool(stray.any()):
        lin = torch.nonzero(stray.reshape(-1))[:, 0].cpu().numpy()
        tiles, trips = tc.locate(plan, scene["dims"], lin)
        pytest.fail(f"{name}: {len(lin)} voxels outside every camera's crop were changed; first in tile {int(tiles[0])}, "
                    f"trip {int(trips[0])}")


# ------------------------------------------------------------------------------------------- 2c ------------------
@pytest.fixture(scope="module")
def default_volume():
    """OurFuser() -- 504^3, the 16 x 16 x 64 form on exactly 8192 tiles -- after the four frames of tc.default_volume_scene:
    three through fuse_frames, the fourth behind its mask through TSDFFuser.integrate_depth."""
    scene = tc.default_volume_scene()
    fuser = OurFuser(device=DEV)
    f = fuser.tsdf_fuser_pred
    assert tuple(f.shape) == scene["dims"] == (504, 504, 504)
    assert (f.min_depth, f.max_depth, f.voxel_size) == (scene["min_depth"], scene["max_depth"], scene["voxel_size"])
    assert np.array_equal(f.tsdf._origin_f32.numpy(), scene["origin"])
    d, K, T = (torch.from_numpy(scene[k]).to(DEV) for k in ("depth", "K", "T"))
    fuser.fuse_frames(d[:3], K[:3], T[:3], None)
    f.integrate_depth(d[3:].half(), T[3:].half(), K[3:].half(), depth_mask_b1hw=_mask(scene, slice(3, 4)))
    yield f.tsdf
    del fuser, f
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", list(tc.DEFAULT_CROPS))
def test_default_volume_crops_vs_oracle(default_volume, name):
    """Crops of the fused default volume against the oracle: the frustum core across tile boundaries, three boxes of voxels
    next to the camera planes (fp16 pixel coordinates overflow there and the reference samples texel 0: the cull must keep
    them), the partial last tiles in x and y, and a box behind the cameras.  These crops pin the indexing of the large form."""
    scene = tc.default_volume_scene()
    lo, hi = tc.DEFAULT_CROPS[name]
    v, w = tc.default_volume_crop(name)
    n = int(tc.touched_mask(v, w).sum())
    assert n == 0 if name == "behind" else n > 1000
    _assert_equal(scene, _crop(default_volume.tsdf_values, lo, hi), _crop(default_volume.tsdf_weights, lo, hi), v, w, lo=lo,
                  nan_cap=1e-4, what=f"crop {name}")


@pytest.mark.parametrize("name", list(tc.DEFAULT_CROPS))
def test_default_volume_crops_vs_explicit_coordinates(default_volume, name):
    """The same crops fused as stand-alone volumes from explicit coordinates (TSDF(coords, -1, 0, ...): the small-tile form,
    never culled -- the form test_tsdf_batch_equals_sequential_and_explicit_coords anchors) equal the big volume's slices."""
    scene = tc.default_volume_scene()
    lo, hi = tc.DEFAULT_CROPS[name]
    coords = torch.from_numpy(tc.crop_coords(scene["origin"], scene["voxel_size"], lo, hi)).to(DEV)
    shape = tuple(coords.shape[1:])
    small = TSDF(coords, -torch.ones(shape, device=DEV), torch.zeros(shape, device=DEV), scene["voxel_size"],
                 torch.from_numpy(scene["origin"]))
    assert not small._generated and tc.tile_plan(shape)["form"] == "small"
    fuser = TSDFFuser(small, min_depth=scene["min_depth"], max_depth=scene["max_depth"])
    fuser.integrate_depth(_half(scene, "depth"), _half(scene, "T"), _half(scene, "K"), depth_mask_b1hw=_mask(scene))
    _assert_equal(scene, _crop(default_volume.tsdf_values, lo, hi), _crop(default_volume.tsdf_weights, lo, hi),
                  small.tsdf_values.cpu().numpy(), small.tsdf_weights.cpu().numpy(), lo=lo, nan_cap=1e-4,
                  what=f"crop {name} vs explicit coordinates")


def test_default_volume_culling_differential(default_volume):
    """All 128 M voxels: the generated-coordinate volume (tile and segment culls on) against a second 504^3 volume built by the
    explicit-coordinate constructor (never culled).  This is a check of the CULLING only -- both sides share the tile walk, so
    an indexing error would cancel; the oracle crops above are what pin the indexing.  About 1.8 GB, freed at the end."""
    scene = tc.default_volume_scene()
    shape = scene["dims"]
    coords = default_volume.voxel_coords
    assert tuple(coords.shape) == (3,) + shape and coords.dtype == torch.float16
    other = TSDF(coords, -torch.ones(shape, dtype=torch.float16, device=DEV),
                 torch.zeros(shape, dtype=torch.float16, device=DEV), scene["voxel_size"], default_volume.origin)
    assert not other._generated and default_volume._generated
    try:
        fuser = TSDFFuser(other, min_depth=scene["min_depth"], max_depth=scene["max_depth"])
        fuser.integrate_depth(_half(scene, "depth"), _half(scene, "T"), _half(scene, "K"), depth_mask_b1hw=_mask(scene))
        same_w = torch.equal(default_volume.tsdf_weights.view(torch.int16), other.tsdf_weights.view(torch.int16))
        same_v = torch.equal(default_volume.tsdf_values.view(torch.int16), other.tsdf_values.view(torch.int16))
        if not (same_v and same_w):
            diff = (default_volume.tsdf_weights.view(torch.int16) != other.tsdf_weights.view(torch.int16)) | \
                   (default_volume.tsdf_values.view(torch.int16) != other.tsdf_values.view(torch.int16))
            lin = torch.nonzero(diff.reshape(-1))[:, 0].cpu().numpy()
            plan = tc.tile_plan(shape)
            tiles, trips = tc.locate(plan, shape, lin)
            pytest.fail(f"{len(lin)} voxels differ between the culled and the unculled volume; first at "
                        f"{np.unravel_index(lin[0], shape)}: tile {int(tiles[0])}, trip {int(trips[0])}")
        assert int((other.tsdf_weights > 0).sum()) > 100000
    finally:
        default_volume._voxel_coords = None
        del other, coords
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------- 2d ------------------
@pytest.mark.parametrize("which", list(tc.RANGE_ORIGINS))
def test_production_numeric_range(which):
    """64^3 at 4 cm with the cameras inside the volume, 640 x 480, f = 577.87, once around the world origin and once around
    (8.4, -9.9, 7.7), where fp16 coordinates are 2^-7 apart: the whole volume against the oracle.  Some touched voxels lie
    outside every frame's frustum: the ones reached through a non-finite pixel coordinate (texel 0)."""
    scene = tc.range_scene(which)
    v, w = tc.oracle_full(scene)
    index = tc.touched_index(v, w)
    assert len(index[0]) > 1000 and int(tc.outside_every_frustum(scene, index).sum()) > 0
    vol = _fuse(scene)
    coords = tc.crop_coords(scene["origin"], scene["voxel_size"], (0, 0, 0), scene["dims"])
    assert np.array_equal(vol.voxel_coords.cpu().numpy().view(np.uint16),
                          np.broadcast_to(coords, (3,) + scene["dims"]).view(np.uint16))
    _assert_equal(scene, vol.tsdf_values, vol.tsdf_weights, v, w, nan_cap=1e-4, what="whole volume")


# ------------------------------------------------------------------------------------------- 2e ------------------
@pytest.mark.parametrize("B", tc.BATCH_SIZES)
def test_frames_per_call(B):
    """300 frames (more than the 256 threads that stride over the frames), 1024 (the most one launch takes: 50 176 bytes of
    dynamic LDS) and 1030 (integrate_depth splits into launches of 1024 and 6; the update is sequential per voxel, so that is
    exact) of 6 x 8 depth maps with distinct poses and a mask into 32^3, against the oracle; no NaN anywhere."""
    scene = tc.first_frames(tc.batch_scene(), B)
    assert len(scene["depth"]) == B and (B <= tc.MAX_FRAMES or B - tc.MAX_FRAMES < 16)
    v, w = tc.batch_oracle()[B]
    vol = _fuse(scene)
    _assert_equal(scene, vol.tsdf_values, vol.tsdf_weights, v, w, what=f"{B} frames in one call")


def test_library_refuses_more_than_1024_frames():
    """The C entry point itself takes at most 1024 frames (TSDFFuser.integrate_depth is what splits), and leaves the volume
    alone when it refuses."""
    scene = tc.first_frames(tc.batch_scene(), tc.MAX_FRAMES + 1)
    vol = TSDF.from_bounds(dict(scene["bounds"]), scene["voxel_size"], device=DEV)
    d, T, K = (_half(scene, k).contiguous() for k in ("depth", "T", "K"))
    o = scene["origin"]
    with pytest.raises(_lib.HipLibraryError):
        _lib.call("sr_tsdf_integrate_fwd", torch.device(DEV), vol.tsdf_values, vol.tsdf_weights, None, 32, 32, 32,
                  float(o[0]), float(o[1]), float(o[2]), scene["voxel_size"], d, None, K, T, tc.MAX_FRAMES + 1, 6, 8,
                  0.25, 3.0, 2.75, 3.0 * scene["voxel_size"], 100.0)
    torch.cuda.synchronize()
    assert bool((vol.tsdf_values == -1).all()) and bool((vol.tsdf_weights == 0).all())
