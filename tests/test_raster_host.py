"""Host-side checks of the mesh rasteriser: the float64 oracle against closed forms, the contested-pixel cap on every
stored scene, render.py's argument validation and the C ABI listing (no GPU needed)."""
import os
import re

import numpy as np
import pytest
import torch

import raster_cases as rc
import raster_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sr_raster_small", "sr_raster_large_setup", "sr_raster_large", "sr_raster_resolve",
           "sr_raster_visibility_mask", "sr_raster_visibility_count")


def _plane_mesh(n, c, extent=40.0):
    """Two big triangles in the plane n . X = c."""
    n = np.asarray(n, np.float64)
    p0 = n * c / (n @ n)
    a = np.cross(n, [0.3, 1.0, 0.1])
    a /= np.linalg.norm(a)
    b = np.cross(n, a)
    b /= np.linalg.norm(b)
    v = np.stack([p0 + extent * (sa * a + sb * b) for sa, sb in ((-1, -1), (1, -1), (1, 1), (-1, 1))])
    return v, np.array([[0, 1, 2], [0, 2, 3]])


@pytest.mark.parametrize("off", rc.OFFSETS)
def test_oracle_fronto_parallel_plane(off):
    H, W = 37, 51
    v, f = _plane_mesh((0.0, 0.0, 1.0), 2.5)
    r = ro.cast(v, f, rc.intrinsics(H, W), np.eye(4), H, W, 0.05, off)
    assert np.array_equal(r["depth"], np.full((H, W), 2.5)) and not r["contested"].any()
    assert np.array_equal(r["d_loose"], r["depth"]) and np.array_equal(r["d_firm"], r["depth"])


@pytest.mark.parametrize("off", rc.OFFSETS)
def test_oracle_tilted_plane(off):
    H, W = 37, 51
    n, c = np.array([0.3, -0.2, 1.0]), 2.0
    v, f = _plane_mesh(n, c)
    K = rc.intrinsics(H, W)
    r = ro.cast(v, f, K, np.eye(4), H, W, 0.05, off)
    want = (c / (ro.rays(K, H, W, off) @ n)).reshape(H, W)
    assert np.abs(r["depth"] - want).max() <= 1e-12 * want.max()
    assert not r["contested"].any()
    # a pose moves the camera, not the answer: the same plane expressed in a world frame
    Tm = np.eye(4)
    Tm[:3, :3] = [[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]]
    Tm[:3, 3] = [0.3, -0.1, 0.2]                          # cam_T_world
    vw = (v - Tm[:3, 3]) @ Tm[:3, :3]                     # world = R^T (cam - t)
    r2 = ro.cast(vw, f, K, Tm, H, W, 0.05, off)
    assert np.abs(r2["depth"] - want).max() <= 1e-12 * want.max()


def test_oracle_near_plane_silhouette_and_ties():
    H, W = 24, 32
    K = rc.intrinsics(H, W)
    # nothing nearer than znear is seen
    v, f = _plane_mesh((0.0, 0.0, 1.0), 0.04)
    assert (ro.cast(v, f, K, np.eye(4), H, W, 0.05, 0.0)["depth"] == 0).all()
    # a small square in front of nothing: hits inside, misses outside, its outline contested only where a pixel
    # sample lies within tau of it
    s = np.array([[-0.2, -0.2, 1.0], [0.2, -0.2, 1.0], [0.2, 0.2, 1.0], [-0.2, 0.2, 1.0]])
    r = ro.cast(s, np.array([[0, 1, 2], [0, 2, 3]]), K, np.eye(4), H, W, 0.05, 0.0)
    u = (np.arange(W) - K[0, 2]) / K[0, 0]
    vv = (np.arange(H) - K[1, 2]) / K[1, 1]
    inside = (np.abs(u)[None, :] <= 0.2) & (np.abs(vv)[:, None] <= 0.2)
    assert np.array_equal(r["depth"] > 0, inside) and inside.any() and not inside.all()
    assert not r["contested"].any()                       # (no sample of this grid is within 1/32 px of the outline)
    # duplicated faces: the lowest index wins
    r = ro.cast(s, np.array([[0, 1, 2], [0, 2, 3], [0, 1, 2]]), K, np.eye(4), H, W, 0.05, 0.0)
    assert set(np.unique(r["face"])) <= {-1, 0, 1}
    # a triangle through the camera plane needs no special case: the floor y = 1 under the camera
    fl = np.array([[-50.0, 1.0, -50.0], [50.0, 1.0, -50.0], [0.0, 1.0, 80.0]])
    r = ro.cast(fl, np.array([[0, 1, 2]]), K, np.eye(4), H, W, 0.05, 0.0)
    below = vv > 0.05
    assert np.allclose(r["depth"][below], np.broadcast_to((1.0 / vv)[:, None], (H, W))[below], rtol=1e-12)
    assert (r["depth"][vv <= 0] == 0).all()


@pytest.mark.parametrize("name", rc.SCENES)
def test_stored_scenes_stay_under_the_contested_cap(name):
    sc = rc.load(name)
    assert sc["vertices"].dtype == np.float32 and sc["faces"].dtype == np.int32 and sc["cam_T_world"].shape == (5, 4, 4)
    for H, W in rc.SIZES:
        for off in rc.OFFSETS:
            r = ro.cast(sc["vertices"], sc["faces"], rc.intrinsics(H, W), sc["cam_T_world"][0], H, W, rc.ZNEAR, off)
            share = r["contested"].mean()
            print(f"{name} {W}x{H} offset {off}: contested {share:.4f}, hit {np.mean(r['depth'] > 0):.3f}")
            assert share <= ro.MAX_CONTESTED_SHARE
            assert (r["depth"] > 0).mean() > 0.2
    if name == "occluder":      # the turned views used by the GPU test
        H, W = rc.SIZES[0]
        for b in range(1, 5):
            r = ro.cast(sc["vertices"], sc["faces"], rc.intrinsics(H, W), sc["cam_T_world"][b], H, W, rc.ZNEAR, 0.0)
            assert r["contested"].mean() <= ro.MAX_CONTESTED_SHARE


def test_scene_properties():
    """What the scenes are there for: small triangles, large ones, junk faces, a triangle through the camera plane."""
    H, W = rc.SIZES[0]
    K = rc.intrinsics(H, W).astype(np.float64)

    def boxes(name):
        sc = rc.load(name)
        tri, ok = ro.camera_triangles(sc["vertices"], sc["faces"], sc["cam_T_world"][0])
        return sc, tri, ok

    sc, tri, ok = boxes("grid")
    assert ok.all() and 4500 <= len(tri) <= 5500
    px = tri[..., :2] / tri[..., 2:] * K[0, 0]
    ext = (px.max(1) - px.min(1)).max(1)
    assert np.median(ext) < 3.0                                       # about a pixel or two across
    sc, tri, ok = boxes("room")
    assert len(tri) == 12 and (tri[..., 2].min(1) < 0).sum() >= 6     # faces behind and through the camera plane
    sc, tri, ok = boxes("near")
    assert (tri[0, :, 2] < 0).sum() == 2 and (tri[0, :, 2] > 0).sum() == 1
    sc, tri, ok = boxes("junk")
    assert (~ok).sum() >= 5 and not np.isfinite(sc["vertices"]).all()
    assert (tri[ok][..., 2].max(1) < 0).any()                         # wholly behind the camera


def test_argument_validation():
    from simplerecon_amd import render
    from simplerecon_amd._lib import HipLibraryError
    from simplerecon_amd.tsdf import TriangleMesh
    v = torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]])
    f = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    K = torch.from_numpy(rc.intrinsics(8, 12))[None]
    T = torch.eye(4)[None]
    mesh = TriangleMesh(v, f)
    for fn in (render.render_depth, render.visible_faces, render.cull_to_visible):
        with pytest.raises(HipLibraryError):
            fn(mesh, K, T, 8, 12)                                    # host tensors: no CPU fallback
        with pytest.raises(ValueError):
            fn(mesh, K, T, 8, 12, cull="front-ish")
        with pytest.raises(ValueError):
            fn(TriangleMesh(v[:, :2], f), K, T, 8, 12)
        with pytest.raises(ValueError):
            fn(TriangleMesh(v, f.reshape(3, 1)), K, T, 8, 12)
        with pytest.raises(TypeError):
            fn(TriangleMesh(v.double(), f), K, T, 8, 12)
        with pytest.raises(TypeError):
            fn(TriangleMesh(v, f.long()), K, T, 8, 12)
        with pytest.raises(TypeError):
            fn((v, f), K, T, 8, 12)
        with pytest.raises(ValueError):
            fn(mesh, K, T, 0, 12)
        with pytest.raises(ValueError):
            fn(mesh, K, T, 8, 12, znear=0.0)
        with pytest.raises(ValueError):
            fn(mesh, K, T, 8, 12, pixel_offset=2.0)
    with pytest.raises(ValueError):
        render.visible_faces(mesh, K, T, 8, 12, min_views=0)
    r = render.Renderer(8, 12)
    with pytest.raises(NotImplementedError):
        r.render_mesh([mesh], 8, 12, np.eye(4), np.eye(3), get_colour=True)
    with pytest.raises(TypeError):
        r.render_mesh([], 8, 12, np.eye(4), np.eye(3))
    assert render.CULL_MODES == {"none": 0, "back": 1}


def test_camera_validation_needs_no_device(monkeypatch):
    """Shapes of the cameras are checked before anything is asked of the GPU."""
    from simplerecon_amd import render
    from simplerecon_amd._lib import HipLibraryError
    with pytest.raises(ValueError):
        render._check_cameras(torch.eye(3)[None], torch.eye(4)[None], torch.device("cpu"))
    with pytest.raises(TypeError):
        render._check_cameras(np.eye(4)[None], torch.eye(4)[None], torch.device("cpu"))
    with pytest.raises(HipLibraryError):
        render._check_cameras(torch.eye(4)[None], torch.eye(4)[None], torch.device("cpu"))


def test_symbols_are_declared_bound_and_exported():
    import ctypes
    from simplerecon_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "simplerecon_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in the header"
        assert name in _lib.SIGNATURES and hasattr(raw, name)
    assert _lib.ABI_VERSION == 5 and raw.sr_abi_version() == 5
    for macro, value in (("SR_RASTER_CULL_NONE", 0), ("SR_RASTER_CULL_BACK", 1), ("SR_RASTER_MAX_SIDE", 32768),
                         ("SR_RASTER_RECORD_BYTES", 80), ("SR_RASTER_MASK_VIEWS", 64)):
        assert re.search(rf"#define {macro} {value}\b", hdr)
    # host-side refusals of the entry points (no launch happens)
    assert raw.sr_raster_resolve(None, ctypes.c_int64(4), None, None, None) == 1
    assert raw.sr_raster_visibility_count(None, ctypes.c_int64(4), None, 1, None, None) == 1
