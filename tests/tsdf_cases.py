"""Case table and launch-plan arithmetic of tests/test_gpu_tsdf_volumes.py: the dense fuser (csrc/sr_tsdf.hip, behind
TSDFFuser.integrate_depth and OurFuser) at the volume sizes where its launch changes form -- a workgroup's second and later
tiles, the 16 x 16 x 64 tile with its walk over 8 sub-bricks, the default 504^3 volume with production intrinsics, batches
of more than 256 and more than 1024 frames -- and the brick / chunk arithmetic of the marching-cubes scan (csrc/sr_mesh.hip)
that tests/test_gpu_mesh.py sizes its large volumes by.

Everything here runs on any device: the GPU module uses it for its scenes, its oracle references and to attribute a mismatch to
(tile, trip); tests/test_tsdf_cases_host.py checks the table, the plans and -- from the numpy oracle alone -- that no case
passes vacuously.

The plan arithmetic RESTATES the launcher on purpose (there is no library query for the tile form):

    big   = ceil(X/16) * ceil(Y/16) * ceil(Z/64)
    tile  = (16, 16, 64) if big >= 8192 else (8, 8, 32)                      sr_tsdf.hip, sr_tsdf_integrate_fwd
    tiles = ceil(X/tx) * ceil(Y/ty) * ceil(Z/tz);   grid = min(tiles, 4096)
    tile index = (txi * nty + tyi) * ntz + tzi;     workgroup g walks tiles g, g + grid, ...: trip of a tile = tile // grid

A scene is dict(name, dims, voxel_size, origin (fp32 [3]), bounds (TSDF.from_bounds gives exactly dims / origin), depth
[B,1,H,W] fp32, K / T [B,4,4] fp32 (intrinsics, cam_T_world), mask ([B,1,H,W] bool or None), min_depth, max_depth); the fuser
and the oracle both round depth, K and T to fp16."""
import functools

import numpy as np

import oracle

GRID_CAP = 4096            # sr_tsdf_integrate_fwd: blocks = min(tiles, 4096)
LARGE_FORM_TILES = 8192    # 16 x 16 x 64 tiles only if there are at least this many of them
SMALL_TILE, LARGE_TILE = (8, 8, 32), (16, 16, 64)
MAX_FRAMES = 1024          # frames per launch: the C entry point refuses more, TSDFFuser.integrate_depth splits


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------- fusion plan ---------
def tile_plan(dims):
    X, Y, Z = dims
    big = cdiv(X, 16) * cdiv(Y, 16) * cdiv(Z, 64)
    large = big >= LARGE_FORM_TILES
    tile = LARGE_TILE if large else SMALL_TILE
    nt = tuple(cdiv(d, t) for d, t in zip(dims, tile))
    tiles = nt[0] * nt[1] * nt[2]
    grid = min(tiles, GRID_CAP)
    return dict(form="large" if large else "small", tile=tile, nt=nt, tiles=tiles, grid=grid, trips=cdiv(tiles, grid),
                large_tiles=big, partial=tuple(d % t for d, t in zip(dims, tile)))


def tile_of(plan, ix, iy, iz):
    """Tile index of voxel (ix, iy, iz); integers or broadcastable integer arrays."""
    (tx, ty, tz), (_, nty, ntz) = plan["tile"], plan["nt"]
    return (ix // tx * nty + iy // ty) * ntz + iz // tz


def trip_of(plan, ix, iy, iz):
    """Which of its workgroup's tiles (0 = the first) holds the voxel."""
    return tile_of(plan, ix, iy, iz) // plan["grid"]


def locate(plan, dims, linear):
    """(tile, trip) of linear voxel indices (z fastest), for error messages."""
    ix, iy, iz = np.unravel_index(np.asarray(linear, np.int64), dims)
    t = tile_of(plan, ix, iy, iz)
    return t, t // plan["grid"]


def dynamic_lds_bytes(B):
    """12 fp32 of H(K @ T) per frame, then the frame flags padded to 16 bytes."""
    return 48 * B + 16 * cdiv(B, 16)


def touched_mask(values, weights):
    """Voxels an integration changed: the volume starts as (-1, 0); an update adds a weight >= 0 and writes a value in
    [-1, 1] (or NaN, where a confidence underflows to a zero weight)."""
    return (np.asarray(weights) != 0) | (np.asarray(values).view(np.uint16) != np.float16(-1).view(np.uint16))


def trip_shares(plan, touched_index):
    """Share of the touched voxels in each trip; touched_index = (ix, iy, iz) arrays of global voxel indices."""
    trips = trip_of(plan, *touched_index)
    return np.bincount(trips, minlength=plan["trips"]) / max(1, len(trips))


def tiles_touched(plan, touched_index):
    return np.unique(tile_of(plan, *touched_index))


# ------------------------------------------------------------------------------------------- mesh plan -----------
def mesh_plan(dims):
    """sr_mesh.hip: a thread owns 8 voxels along z, a brick is 256 threads; sr_mesh_scan_kernel gives each of its 1024 threads
    `chunk` consecutive bricks, so only the first ceil(nbricks / chunk) threads have any."""
    X, Y, Z = dims
    groups = X * Y * cdiv(Z, 8)
    nbricks = cdiv(groups, 256)
    chunk = cdiv(nbricks, 1024)
    return dict(groups=groups, nbricks=nbricks, chunk=chunk, busy_threads=cdiv(nbricks, chunk))


# ------------------------------------------------------------------------------------------- coordinates ---------
def crop_coords(origin_f32, voxel_size, lo, hi):
    """fp16 [3,x,y,z] world coordinates of voxels lo <= index < hi of a generated volume, without the full grid:
    per axis H(origin + index * voxel_size) in fp32 (generate_voxel_coords, then .half())."""
    o = np.asarray(origin_f32, np.float32)
    shape = tuple(h - l for l, h in zip(lo, hi))
    out = np.empty((3,) + shape, np.float16)
    for a in range(3):
        line = (o[a] + np.arange(lo[a], hi[a]).astype(np.float32) * np.float32(voxel_size)).astype(np.float16)
        view = [1, 1, 1]
        view[a] = shape[a]
        out[a] = line.reshape(view)
    return out


def bounds_for(origin, dims, voxel_size):
    """Bounds from which TSDF.from_bounds / oracle.tsdf_from_bounds derive exactly `dims`: half a rounding unit (4 voxels)
    short of the full extent, so that the ceil in from_bounds cannot fall on either side of an integer."""
    b = {}
    for i, a in enumerate("xyz"):
        b[a + "min"] = float(origin[i])
        b[a + "max"] = float(origin[i]) + (dims[i] - 4) * voxel_size
    return b


def oracle_crop(scene, lo, hi):
    """(values, weights) of the crop lo <= index < hi after the scene's frames, by the numpy oracle."""
    coords = crop_coords(scene["origin"], scene["voxel_size"], lo, hi)
    shape = coords.shape[1:]
    v, w = -np.ones(shape, np.float16), np.zeros(shape, np.float16)
    oracle.tsdf_integrate(v, w, coords, scene["depth"], scene["T"], scene["K"], min_depth=scene["min_depth"],
                          max_depth=scene["max_depth"], voxel_size=scene["voxel_size"], depth_mask_b1hw=scene["mask"])
    return v, w


def oracle_full(scene):
    return oracle_crop(scene, (0, 0, 0), scene["dims"])


def touched_index(v, w, lo=(0, 0, 0)):
    return tuple(i + l for i, l in zip(np.nonzero(touched_mask(v, w)), lo))


# ------------------------------------------------------------------------------------------- scene parts ---------
def intrinsics(n, f, cx, cy):
    K = np.tile(np.eye(4, dtype=np.float32), (n, 1, 1))
    K[:, 0, 0] = K[:, 1, 1] = f
    K[:, 0, 2], K[:, 1, 2] = cx, cy
    return K


def rot_y(deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])


def rot_x(deg):
    c, s = np.cos(np.deg2rad(deg)), np.sin(np.deg2rad(deg))
    return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])


def extrinsics(centres, rotations=None):
    """cam_T_world of cameras at `centres` whose axes are the columns of `rotations` (world_R_cam; default identity: the camera
    looks down +z)."""
    T = np.tile(np.eye(4, dtype=np.float32), (len(centres), 1, 1))
    for i, c in enumerate(centres):
        R = np.eye(3) if rotations is None else np.asarray(rotations[i]).T
        T[i, :3, :3] = R
        T[i, :3, 3] = -R @ np.asarray(c, np.float64)
    return T


def _scene(name, dims, voxel_size, origin, depth, K, T, mask, min_depth, max_depth):
    origin = np.asarray(origin, np.float32)
    return dict(name=name, dims=tuple(dims), voxel_size=voxel_size, origin=origin, bounds=bounds_for(origin, dims, voxel_size),
                depth=depth.astype(np.float32), K=K, T=T, mask=mask, min_depth=min_depth, max_depth=max_depth)


def _block_mask(rng, B, H, W, frame, block, keep=0.7):
    """All true, except random blocks of one frame."""
    mask = np.ones((B, 1, H, W), bool)
    coarse = rng.random((cdiv(H, block), cdiv(W, block))) < keep
    mask[frame, 0] = np.repeat(np.repeat(coarse, block, 0), block, 1)[:H, :W]
    return mask


# ------------------------------------------------------------------------------------------- 2a / 2b: slabs ------
# A thin slab seen from 1 m by cameras looking down +z (48 x 64 images, f = 40): each camera's frustum covers about 92 x 68
# columns of 2 cm voxels, so where the camera centres lie decides which tiles -- and which trips -- are updated.
SLAB_H, SLAB_W, SLAB_F = 48, 64, 40.0
SLAB_MIN_DEPTH, SLAB_MAX_DEPTH = 0.25, 3.0


def _slab_scene(name, dims, z0, centres_xy, seed, mask_frame):
    vs = 0.02
    origin = (-dims[0] * vs / 2, -dims[1] * vs / 2, z0)
    rng = np.random.default_rng(seed)
    B = len(centres_xy)
    mid = z0 + dims[2] * vs / 2
    depth = mid + rng.uniform(-0.05, 0.05, (B, 1, SLAB_H, SLAB_W))
    K = intrinsics(B, SLAB_F, SLAB_W / 2, SLAB_H / 2)
    T = extrinsics([(x, y, 0.0) for x, y in centres_xy])
    mask = None if mask_frame is None else _block_mask(rng, B, SLAB_H, SLAB_W, mask_frame, 8)
    s = _scene(name, dims, vs, origin, depth, K, T, mask, SLAB_MIN_DEPTH, SLAB_MAX_DEPTH)
    s["centres_xy"] = list(centres_xy)
    return s


def slab_crop_box(scene, centre_xy, margin=4):
    """The box (lo, hi) of voxel indices that the camera at `centre_xy` can update: the image-corner rays at the slab's far
    face, plus `margin` voxels, clipped to the volume; the whole z extent.  None if the frustum misses the volume."""
    vs, dims, o = scene["voxel_size"], scene["dims"], scene["origin"].astype(np.float64)
    zfar = o[2] + (dims[2] - 1) * vs
    half = (SLAB_W / 2 / SLAB_F * zfar, SLAB_H / 2 / SLAB_F * zfar)
    lo, hi = [0, 0, 0], [0, 0, dims[2]]
    for a in range(2):
        lo[a] = max(0, int(np.floor((centre_xy[a] - half[a] - o[a]) / vs)) - margin)
        hi[a] = min(dims[a], int(np.ceil((centre_xy[a] + half[a] - o[a]) / vs)) + 1 + margin)
        if lo[a] >= hi[a]:
            return None
    return tuple(lo), tuple(hi)


def slab_min_voxel_depth(scene):
    """Smallest camera-space depth of any voxel: all cameras stand at z = 0 and look down +z, so it is the fp16 z coordinate of
    the first voxel layer -- far above the 0.25 m below which the kernel stops culling by pixel position."""
    return float(np.float16(scene["origin"][2]))


def _idx_to_world(dims, idx, a, vs=0.02):
    return (idx - dims[a] / 2) * vs


@functools.lru_cache(maxsize=None)
def slab_case(name):
    if name == "two_trips_8190":
        # 90 x 91 x 1 small tiles; trip 1 = tiles >= 4096 = x index >= 360 (x >= 0)
        return _slab_scene(name, (720, 728, 8), 1.0, [(-4.0, 0.3), (4.0, -2.1), (6.5, 1.7)], 11, 1)
    if name == "two_z_tiles_5100":
        # 50 x 51 x 2 small tiles, the second z-tile holds 8 of 32 voxels; trip 1 = x index >= 320 and a bit (x >= 2.4)
        return _slab_scene(name, (400, 408, 40), 0.6, [(-1.5, 0.5), (2.4, -1.0), (3.2, 2.2)], 12, 2)
    if name == "below_threshold_small":
        # 180 x 181 small tiles in 8 trips of 22.6 tile rows (181 voxels of x) each: four cameras straddle the boundaries
        # between trips 0|1, 2|3, 4|5, 6|7, one hangs over the x-max face, one over the y-max face
        d = (1440, 1448, 8)
        cx = [_idx_to_world(d, 181 * k, 0) for k in (1, 3, 5, 7)]
        return _slab_scene(name, d, 1.0, [(cx[0], -9.0), (cx[1], 3.1), (cx[2], -2.2), (cx[3], 8.05),
                                          (_idx_to_world(d, 1440 + 25, 0), -6.0), (-11.0, _idx_to_world(d, 1448 + 10, 1))],
                           13, 3)
    if name == "at_threshold_large":
        # 91 x 91 tiles of 16 x 16 x 64 on 4096 workgroups: trip 1 from x index 720, trip 2 = the partial last tile row in x
        # (x index 1440..1447) from y index 32.  One camera straddles x index 720, three hang over the x-max face so that
        # half of what they touch is in trip 2, one hangs over the y-max face (partial last tile in y) and one over the corner
        d = (1448, 1448, 8)
        over_x, over_y = _idx_to_world(d, 1448 + 30, 0), _idx_to_world(d, 1448 + 10, 1)
        return _slab_scene(name, d, 1.0, [(_idx_to_world(d, 720, 0), -5.3), (-8.0, over_y), (over_x, -9.1), (over_x, -1.0),
                                          (over_x, 6.2), (over_x, over_y)], 14, 4)
    raise KeyError(name)


SLAB_FULL = ("two_trips_8190", "two_z_tiles_5100")               # 2a: full-volume oracle
SLAB_CROPS = ("below_threshold_small", "at_threshold_large")     # 2b: one oracle crop per camera


@functools.lru_cache(maxsize=None)
def slab_crops(name):
    """[(lo, hi, values, weights)] of a 2b case: the oracle (all frames) on every camera's box."""
    scene = slab_case(name)
    out = []
    for c in scene["centres_xy"]:
        box = slab_crop_box(scene, c)
        assert box is not None, f"{name}: the camera at {c} cannot see the volume"
        out.append(box + oracle_crop(scene, *box))
    return out


def crop_reaches_outer_layer(scene, lo, hi, v, w):
    """Whether a touched voxel lies on a face of the crop that is not a face of the volume."""
    t = touched_mask(v, w)
    hit = False
    for a in range(3):
        sl = [slice(None)] * 3
        if lo[a] > 0:
            sl[a] = 0
            hit |= bool(t[tuple(sl)].any())
        if hi[a] < scene["dims"][a]:
            sl[a] = -1
            hit |= bool(t[tuple(sl)].any())
    return hit


# ------------------------------------------------------------------------------------------- 2c: default volume --
PROD_H, PROD_W, PROD_F = 480, 640, 577.87
DEFAULT_CROPS = {
    # name: (lo, hi); every crop is at most 1 M voxels and a multiple of 8 deep (it is also fused on its own)
    "core": ((200, 200, 250), (304, 304, 330)),            # the frusta, across tile boundaries in x, y (16) and z (256, 320)
    "plane_far_corner": ((480, 480, 248), (504, 504, 256)),   # voxels next to the camera plane, 14 m from the optical axis:
    "plane_near_corner": ((0, 0, 248), (24, 24, 256)),        # fp16 pixel coordinates overflow, the reference samples texel 0
    "plane_x_axis": ((400, 200, 240), (480, 304, 272)),
    "last_tiles_x": ((496, 0, 240), (504, 504, 272)),      # 504 = 31 * 16 + 8: the partial last tiles in x
    "last_tiles_y": ((0, 496, 240), (504, 504, 272)),      # ... and in y
    "behind": ((200, 200, 152), (304, 304, 224)),          # behind every camera: nothing may change
}


@functools.lru_cache(maxsize=None)
def default_volume_scene():
    """OurFuser()'s volume, +-10 m at 4 cm (504^3), four 640 x 480 frames from around the volume's centre: identity, two small
    translations, one of them rotated 20 degrees about y; the last frame behind a mask that also hides texel 0."""
    rng = np.random.default_rng(21)
    B = 4
    coarse = 1.0 + 1.5 * rng.random((B, 1, 48, 64))
    depth = np.repeat(np.repeat(coarse, 10, 2), 10, 3)
    centres = [(0.0, 0.0, 0.0), (0.1, -0.05, 0.05), (-0.15, 0.02, 0.03), (-0.08, 0.06, 0.0)]
    T = extrinsics(centres, [np.eye(3), np.eye(3), rot_y(20.0), np.eye(3)])
    mask = _block_mask(rng, B, PROD_H, PROD_W, 3, 40)
    mask[3, 0, :40, :40] = False
    return _scene("default_504", (504, 504, 504), 0.04, (-10.0, -10.0, -10.0), depth,
                  intrinsics(B, PROD_F, 320.0, 240.0), T, mask, 0.5, 3.0)


@functools.lru_cache(maxsize=None)
def default_volume_crop(name):
    lo, hi = DEFAULT_CROPS[name]
    return oracle_crop(default_volume_scene(), lo, hi)


# ------------------------------------------------------------------------------------------- 2d: numeric range ---
RANGE_ORIGINS = {"near": (-1.28, -1.28, -1.28), "far": (8.4, -9.9, 7.7)}   # far: fp16 coordinates have 2^-7 spacing


@functools.lru_cache(maxsize=None)
def range_scene(which):
    """64^3 at 4 cm with the cameras inside the volume, 640 x 480, f = 577.87: voxels on and next to the camera planes."""
    rng = np.random.default_rng(31)
    B = 3
    o = np.asarray(RANGE_ORIGINS[which], np.float64)
    coarse = 0.6 + 1.4 * rng.random((B, 1, 48, 64))
    depth = np.repeat(np.repeat(coarse, 10, 2), 10, 3)
    centres = [o + (1.3, 1.22, 0.5), o + (1.1, 1.3, 0.62), o + (1.45, 1.1, 0.41)]
    T = extrinsics(centres, [np.eye(3), rot_y(12.0), rot_x(-9.0)])
    return _scene("range_" + which, (64, 64, 64), 0.04, o, depth, intrinsics(B, PROD_F, 320.0, 240.0), T, None, 0.5, 3.0)


def outside_every_frustum(scene, index):
    """Of the voxels `index` = (ix, iy, iz): which lie outside every frame's view frustum in exact geometry (float64, on the
    fp16-rounded inputs), by a margin (20 cm sideways at twice the image's half-angle) that no fp16 rounding of the projection
    chain can bridge.  A voxel the fuser still updates there was reached through a non-finite pixel coordinate (texel 0)."""
    coords = crop_coords(scene["origin"], scene["voxel_size"], (0, 0, 0), scene["dims"]).astype(np.float64)
    p = np.stack([np.broadcast_to(coords[a], scene["dims"])[index] for a in range(3)] + [np.ones(len(index[0]))], 0)
    outside = np.ones(len(index[0]), bool)
    for b in range(len(scene["T"])):
        K = scene["K"][b].astype(np.float16).astype(np.float64)
        cam = scene["T"][b].astype(np.float16).astype(np.float64) @ p
        x, y, z = cam[0], cam[1], cam[2]
        inside = (z > 0) & (np.abs(x) <= 2 * (scene["depth"].shape[3] / 2 / K[0, 0]) * z + 0.2) \
            & (np.abs(y) <= 2 * (scene["depth"].shape[2] / 2 / K[1, 1]) * z + 0.2)
        outside &= ~inside
    return outside


# ------------------------------------------------------------------------------------------- 2e: frames per call -
BATCH_SIZES = (300, 1024, 1030)    # more than the 256 threads that stride over the frames; the most one launch takes; a split


@functools.lru_cache(maxsize=None)
def batch_scene():
    """1030 frames of 6 x 8 depth maps with distinct poses into 32^3 at 5 cm; a mask over all frames."""
    rng = np.random.default_rng(41)
    B, H, W = max(BATCH_SIZES), 6, 8
    depth = 0.8 + rng.random((B, 1, H, W))
    centres = np.concatenate([rng.uniform(-0.3, 0.3, (B, 2)), rng.uniform(-0.3, 0.0, (B, 1))], 1)
    rots = [rot_y(a) @ rot_x(c) for a, c in rng.uniform(-10, 10, (B, 2))]
    mask = rng.random((B, 1, H, W)) < 0.8
    return _scene("batch_32", (32, 32, 32), 0.05, (-0.8, -0.8, 0.5), depth, intrinsics(B, 6.0, W / 2, H / 2),
                  extrinsics(centres, rots), mask, 0.25, 3.0)


def first_frames(scene, n):
    s = dict(scene)
    for k in ("depth", "K", "T", "mask"):
        s[k] = None if scene[k] is None else scene[k][:n]
    return s


@functools.lru_cache(maxsize=None)
def batch_oracle():
    """{B: (values, weights)} for every B of BATCH_SIZES: the oracle is sequential in the frames, so one pass gives all."""
    scene = batch_scene()
    coords = crop_coords(scene["origin"], scene["voxel_size"], (0, 0, 0), scene["dims"])
    v, w = -np.ones(scene["dims"], np.float16), np.zeros(scene["dims"], np.float16)
    out, done = {}, 0
    for B in sorted(BATCH_SIZES):
        oracle.tsdf_integrate(v, w, coords, scene["depth"][done:B], scene["T"][done:B], scene["K"][done:B],
                              min_depth=scene["min_depth"], max_depth=scene["max_depth"], voxel_size=scene["voxel_size"],
                              depth_mask_b1hw=scene["mask"][done:B])
        out[B], done = (v.copy(), w.copy()), B
    return out
