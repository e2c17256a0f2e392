"""The mesh rasteriser (simplerecon_amd/render.py, csrc/sr_raster.hip) against the float64 ray caster of
tests/raster_oracle.py on the stored scenes, plus reproducibility, culling, visibility, the two extreme workloads and
the closed loop depth -> fusion -> mesh -> render."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import raster_cases as rc
import raster_oracle as ro
from simplerecon_amd import _lib, synthetic
from simplerecon_amd.render import Renderer, cull_to_visible, render_depth, visible_faces
from simplerecon_amd.tsdf import OurFuser, TriangleMesh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
_ORACLE = {}


def _mesh(sc):
    return TriangleMesh(torch.from_numpy(sc["vertices"]).to(DEV), torch.from_numpy(sc["faces"]).to(DEV))


def _cams(sc, H, W, views=slice(0, 1)):
    T = torch.from_numpy(sc["cam_T_world"][views]).to(DEV)
    K = torch.from_numpy(rc.intrinsics(H, W))[None].repeat(T.shape[0], 1, 1).to(DEV)
    return K, T


def _oracle(name, H, W, off, view=0):
    key = (name, H, W, off, view)
    if key not in _ORACLE:
        sc = rc.load(name)
        _ORACLE[key] = ro.cast(sc["vertices"], sc["faces"], rc.intrinsics(H, W), sc["cam_T_world"][view], H, W, rc.ZNEAR, off)
    return _ORACLE[key]


def _assert_agrees(depth, want, tag):
    """Uncontested pixels: the same hit / miss and depth within 1e-4 relative.  Figures are printed first."""
    ok = ~want["contested"]
    hit_w, hit_g = want["depth"] > 0, depth > 0
    flips = int((hit_w != hit_g)[ok].sum())
    both = ok & hit_w & hit_g
    rel = np.abs(depth - want["depth"])[both] / want["depth"][both]
    print(f"\n{tag}: contested {want['contested'].mean():.4f}, hit/miss flips {flips}, "
          f"max rel depth err {rel.max() if rel.size else 0.0:.3e} over {int(both.sum())} pixels")
    assert flips == 0
    assert rel.size == 0 or rel.max() <= ro.DEPTH_RTOL


@pytest.mark.parametrize("name,H,W,off", rc.configs())
def test_matches_oracle(name, H, W, off):
    sc = rc.load(name)
    want = _oracle(name, H, W, off)
    assert want["contested"].mean() <= ro.MAX_CONTESTED_SHARE        # a condition on the scene, before the GPU is asked
    K, T = _cams(sc, H, W)
    depth, face = render_depth(_mesh(sc), K, T, H, W, znear=rc.ZNEAR, pixel_offset=off, return_faces=True)
    assert depth.shape == (1, 1, H, W) and depth.dtype == torch.float32
    assert face.shape == (1, H, W) and face.dtype == torch.int32
    depth, face = depth[0, 0].cpu().numpy(), face[0].cpu().numpy()
    assert ((face >= 0) == (depth > 0)).all() and face.max() < len(sc["faces"])
    _assert_agrees(depth, want, f"{name} {W}x{H} offset {off}")
    # face ids: the named face covers the pixel (at one of the five sample points) at the winner's depth
    fd, cov = ro.face_depths(sc["vertices"], sc["faces"], rc.intrinsics(H, W), sc["cam_T_world"][0], H, W, face, rc.ZNEAR, off)
    m = ~want["contested"] & (face >= 0)
    assert cov[m].all()
    assert (np.abs(fd - want["depth"])[m] <= ro.DEPTH_RTOL * want["depth"][m]).all()


def test_other_views_match_oracle():
    """The four turned views of the occluder scene (silhouettes at every angle)."""
    sc = rc.load("occluder")
    H, W = rc.SIZES[0]
    K, T = _cams(sc, H, W, slice(0, 5))
    depth = render_depth(_mesh(sc), K, T, H, W, znear=rc.ZNEAR)[:, 0].cpu().numpy()
    for b in range(1, 5):
        want = _oracle("occluder", H, W, 0.0, b)
        assert want["contested"].mean() <= ro.MAX_CONTESTED_SHARE
        _assert_agrees(depth[b], want, f"occluder view {b}")


def test_reproducible_and_batch_invariant():
    H, W = rc.SIZES[1]
    for name in ("occluder", "junk", "near"):
        sc = rc.load(name)
        mesh = _mesh(sc)
        K, T = _cams(sc, H, W, slice(0, 5))
        d0, f0 = render_depth(mesh, K, T, H, W, return_faces=True)
        d1, f1 = render_depth(mesh, K, T, H, W, return_faces=True)
        assert torch.equal(d0.view(torch.int32), d1.view(torch.int32)) and torch.equal(f0, f1)
        for b in range(5):
            db, fb = render_depth(mesh, K[b:b + 1], T[b:b + 1], H, W, return_faces=True)
            assert torch.equal(db.view(torch.int32), d0[b:b + 1].view(torch.int32)) and torch.equal(fb, f0[b:b + 1])


def _box(lo, hi, inward):
    vs, ts = synthetic._box_faces(np.asarray(lo, float), np.asarray(hi, float), 10.0, inward=inward)
    v = torch.from_numpy(np.concatenate(vs).astype(np.float32)).to(DEV)
    f = torch.from_numpy(np.concatenate(ts).astype(np.int32)).to(DEV)
    return TriangleMesh(v, f)


def test_culling():
    H, W = 72, 96
    K = torch.from_numpy(rc.intrinsics(H, W))[None].to(DEV)
    T = torch.eye(4, device=DEV)[None].clone()
    # a closed box with outward normals, seen from outside
    box = _box((-0.5, -0.4, 1.5), (0.6, 0.5, 2.5), inward=False)
    a = render_depth(box, K, T, H, W, cull="none")
    b = render_depth(box, K, T, H, W, cull="back")
    assert (a > 0).any() and (a == 0).any()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the camera inside a room: inward normals render, flipped winding (outward normals) renders empty
    inside = _box((-2.0, -1.5, -2.0), (2.0, 1.5, 2.0), inward=True)
    flipped = TriangleMesh(inside.vertices, inside.faces.flip(1).contiguous())
    assert (render_depth(inside, K, T, H, W, cull="back") > 0).all()
    assert torch.equal(render_depth(inside, K, T, H, W, cull="back").view(torch.int32),
                       render_depth(inside, K, T, H, W, cull="none").view(torch.int32))
    assert (render_depth(flipped, K, T, H, W, cull="back") == 0).all()
    assert (render_depth(flipped, K, T, H, W, cull="none") > 0).all()


def test_visibility_and_cull_to_visible():
    sc = rc.load("occluder")
    H, W = rc.SIZES[0]
    mesh = _mesh(sc)
    mesh.colors = torch.rand((mesh.vertices.shape[0], 3), device=DEV)
    mesh.normals = torch.nn.functional.normalize(torch.randn((mesh.vertices.shape[0], 3), device=DEV), dim=1)
    K, T = _cams(sc, H, W)
    want = _oracle("occluder", H, W, 0.0)
    vis = visible_faces(mesh, K, T, H, W, znear=rc.ZNEAR)
    assert vis.dtype == torch.bool and vis.shape == (len(sc["faces"]),)
    vis_np = vis.cpu().numpy()
    assert len(sc["hidden"]) > 100 and not vis_np[sc["hidden"]].any()
    seen, counts = np.unique(want["face"][~want["contested"] & (want["face"] >= 0)], return_counts=True)
    assert len(seen[counts >= 4]) > 50 and vis_np[seen[counts >= 4]].all()
    culled = cull_to_visible(mesh, K, T, H, W, znear=rc.ZNEAR)
    nv = culled.vertices.shape[0]
    assert culled.faces.shape[0] == int(vis.sum()) and culled.faces.dtype == torch.int32
    assert int(culled.faces.min()) == 0 and int(culled.faces.max()) == nv - 1
    assert torch.unique(culled.faces).numel() == nv                       # no unreferenced vertex
    assert culled.colors.shape == (nv, 3) and culled.normals.shape == (nv, 3)
    kept = torch.nonzero(vis)[:, 0]
    assert torch.equal(culled.vertices[culled.faces.long()], mesh.vertices[mesh.faces[kept].long()])
    assert torch.equal(culled.colors[culled.faces.long()], mesh.colors[mesh.faces[kept].long()])
    a = render_depth(mesh, K, T, H, W, znear=rc.ZNEAR)[0, 0].cpu().numpy()
    b = render_depth(culled, K, T, H, W, znear=rc.ZNEAR)[0, 0].cpu().numpy()
    ok = ~want["contested"]
    assert np.array_equal(a[ok], b[ok])
    # min_views: over five views, fewer faces are seen twice than once, and all of those are seen once
    K5, T5 = _cams(sc, H, W, slice(0, 5))
    v1 = visible_faces(mesh, K5, T5, H, W, min_views=1)
    v2 = visible_faces(mesh, K5, T5, H, W, min_views=2)
    v6 = visible_faces(mesh, K5, T5, H, W, min_views=6)
    assert int(v2.sum()) < int(v1.sum()) and bool((v1 | ~v2).all()) and not bool(v6.any())
    per_view = torch.stack([visible_faces(mesh, K5[b:b + 1], T5[b:b + 1], H, W) for b in range(5)]).sum(0)
    assert torch.equal(v2, per_view >= 2) and torch.equal(v1, per_view >= 1)


def test_refusals_on_the_device():
    sc = rc.load("room")
    H, W = rc.SIZES[0]
    mesh = _mesh(sc)
    K, T = _cams(sc, H, W)
    bad = TriangleMesh(mesh.vertices, mesh.faces.clone())
    bad.faces[3, 1] = mesh.vertices.shape[0]
    with pytest.raises(ValueError):
        render_depth(bad, K, T, H, W)
    bad.faces[3, 1] = -1
    with pytest.raises(ValueError):
        render_depth(bad, K, T, H, W)
    skew = K.clone()
    skew[0, 0, 1] = 0.5
    with pytest.raises(ValueError):
        render_depth(mesh, skew, T, H, W)
    with pytest.raises(_lib.HipLibraryError):
        render_depth(mesh, K.cpu(), T, H, W)
    empty = TriangleMesh(mesh.vertices, mesh.faces[:0])
    d, f = render_depth(empty, K, T, H, W, return_faces=True)
    assert (d == 0).all() and (f == -1).all()


def test_renderer_matches_render_depth():
    sc = rc.load("occluder")
    H, W = rc.SIZES[0]
    mesh = _mesh(sc)
    K, T = _cams(sc, H, W)
    r = Renderer(height=H, width=W)
    pose = np.linalg.inv(sc["cam_T_world"][0].astype(np.float64))
    got = r.render_mesh([mesh], H, W, pose, rc.intrinsics(H, W)[:3, :3])
    assert isinstance(got, np.ndarray) and got.shape == (H, W) and got.dtype == np.float32
    want = _oracle("occluder", H, W, 0.5)     # every face of this scene faces view 0: culling changes nothing
    _assert_agrees(got, want, "Renderer.render_mesh")
    with pytest.raises(NotImplementedError):
        r.render_mesh([mesh], H, W, pose, rc.intrinsics(H, W), get_colour=True)


def _extreme(case, limit):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(HERE), HERE, os.environ.get("PYTHONPATH", "")]))
    out = subprocess.run([sys.executable, os.path.join(HERE, "raster_extremes.py"), case, "3"], capture_output=True,
                         text=True, timeout=limit, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print("\n" + json.dumps(res))
    return res


def test_both_extremes_finish():
    """Two triangles over a 1920 x 1440 frame and more than a million small faces into 8 views of 640 x 480, each in a
    child process under its own time limit; plausibility only.  Per pixel the full-frame case may not be more than ten
    times slower than the million-face one: beyond that a thread is walking a frame-sized box."""
    full = _extreme("full_frame", 240)
    assert full["hit_share"] == 1.0 and full["max_rel_err"] <= ro.DEPTH_RTOL
    mil = _extreme("million", 420)
    assert mil["faces"] >= 1_000_000
    assert mil["inner_hit_share"] == 1.0 and mil["outside_hit_share"] == 0.0
    assert mil["inner_max_abs_err"] < mil["voxel"]           # analytic sphere depth within one voxel
    assert full["ns_per_pixel"] <= 10.0 * mil["ns_per_pixel"]


def test_closed_loop_fusion_to_render():
    """Noise-free depth -> OurFuser at 0.04 m -> mesh -> render at the fused cameras (pixel_offset 0).  The trilinear
    zero crossing of a TSDF fused from exact depth lies within a voxel of the surface: median |render - input| below
    0.04 m over pixels valid in both, and at least 90 % of the input pixels inside the fusion depth range are hit."""
    N, h, w, vox = 24, 192, 256, 0.04
    sc = synthetic.raycast_scene(N, h, w, seed=2, device=DEV)
    K = torch.eye(4, device=DEV).repeat(N, 1, 1)
    K[:, :3, :3] = sc["K"]
    T = sc["cam_T_world"].contiguous()
    depth = sc["depths"][:, None].contiguous()
    fuser = OurFuser(bounds=dict(xmin=-3.0, xmax=3.0, ymin=-2.0, ymax=2.0, zmin=-3.0, zmax=3.0), fusion_resolution=vox,
                     max_fusion_depth=3.0, device=DEV)
    for i in range(0, N, 8):
        fuser.fuse_frames(depth[i:i + 8], K[i:i + 8], T[i:i + 8])
    mesh = fuser.get_mesh()
    render = render_depth(mesh, K, T, h, w, pixel_offset=0.0)
    lo, hi = fuser.tsdf_fuser_pred.min_depth, fuser.tsdf_fuser_pred.max_depth
    in_range = (depth >= lo) & (depth <= hi)
    both = in_range & (render > 0)
    median = float((render - depth).abs()[both].median())
    coverage = float(both.sum()) / float(in_range.sum())
    print(f"\nclosed loop: {mesh.faces.shape[0]} faces, median |render - input| {median:.4f} m, coverage {coverage:.4f}")
    assert median < vox
    assert coverage >= 0.90
