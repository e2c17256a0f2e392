"""The mesh shading kernels (simplerecon_amd/render.py, csrc/sr_shade.hip) against their float64 restatement
(tests/shade_oracle.py) on the stored rasteriser scenes, plus exactness, determinism, two-sidedness, the light count,
the Renderer wrappers and the example's --render.

Tolerance.  Both sides compute in float64 from the same fp32 inputs and round to fp32 once, so they differ by the
rounding of a value of magnitude <= 1 to fp32 (6e-8) plus float64 noise: 1e-6 absolute leaves room for another order
of operations.  The oracle is fed the GPU's own face image, so silhouettes are not contested here."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import raster_cases as rc
import raster_oracle as ro
import shade_oracle as so
from simplerecon_amd import render
from simplerecon_amd.tsdf import TriangleMesh

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-6
MIN_SMOOTH_LENGTH = 0.05
BACKGROUND = (0.25, 0.5, 0.75)
AMBIENT = 0.2
SHADINGS = (("unlit", so.UNLIT), ("normals", so.NORMALS), ("lambert", so.LAMBERT))
NORMAL_MODES = (("smooth", so.SMOOTH), ("flat", so.FLAT))
_SCENES = {}


def _scene(name):
    """The stored scene with fixed pseudo-random colours, its device mesh (normals from vertex_normals) and lights."""
    if name not in _SCENES:
        sc = rc.load(name)
        colors = np.random.default_rng(7).random((len(sc["vertices"]), 3)).astype(np.float32)
        mesh = TriangleMesh(torch.from_numpy(sc["vertices"]).to(DEV), torch.from_numpy(sc["faces"]).to(DEV), None,
                            torch.from_numpy(colors).to(DEV))
        mesh.normals = render.vertex_normals(mesh)
        T0 = sc["cam_T_world"][0].astype(np.float64)
        centre = -T0[:3, :3].T @ T0[:3, 3]                       # camera centre of view 0, world frame
        lights = np.concatenate([render.directional_light((0.3, 0.5, 0.8), intensity=0.5),
                                 render.point_light(centre + (0.3, -0.2, 0.1), color=(1.0, 0.8, 0.6), intensity=1.5),
                                 render.headlight(color=(0.5, 0.7, 1.0), intensity=0.3)])
        _SCENES[name] = dict(sc=sc, colors=colors, mesh=mesh, normals=mesh.normals.cpu().numpy(), lights=lights)
    return _SCENES[name]


def _cams(sc, H, W, views=slice(0, 1)):
    T = torch.from_numpy(sc["cam_T_world"][views]).to(DEV)
    K = torch.from_numpy(rc.intrinsics(H, W))[None].repeat(T.shape[0], 1, 1).to(DEV)
    return K, T


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _compare(got, want, keep, tag):
    err = np.abs(got.astype(np.float64) - want)[:, keep]
    worst = float(err.max()) if err.size else 0.0
    print(f"{tag}: max abs err {worst:.3e} over {int(keep.sum())} pixels")
    return worst


@pytest.mark.parametrize("name,H,W,off", rc.configs())
def test_matches_oracle(name, H, W, off):
    s = _scene(name)
    sc, mesh = s["sc"], s["mesh"]
    K, T = _cams(sc, H, W)
    Kn, Tn = rc.intrinsics(H, W), sc["cam_T_world"][0]
    _, face = render.render_depth(mesh, K, T, H, W, znear=rc.ZNEAR, pixel_offset=off, return_faces=True)
    face = face[0].cpu().numpy()
    worst = 0.0
    print()
    for nm_name, nm in NORMAL_MODES:
        got_n = render.render_normals(mesh, K, T, H, W, normals=nm_name, znear=rc.ZNEAR, pixel_offset=off)
        assert got_n.shape == (1, 3, H, W) and got_n.dtype == torch.float32
        for sh_name, sh in SHADINGS:
            want = so.shade(sc["vertices"], sc["faces"], Kn, Tn, H, W, off, face, colors=s["colors"], normals=s["normals"],
                            background=BACKGROUND, ambient=AMBIENT, lights=s["lights"], shading=sh, normal_mode=nm)
            assert np.array_equal(want["hit"], face >= 0)
            left_out = want["hit"] & ((want["grazing"] < ro.GRAZING) | ~(want["smooth_length"] >= MIN_SMOOTH_LENGTH))
            assert left_out.mean() <= ro.MAX_CONTESTED_SHARE
            keep = ~left_out
            got = render.render_color(mesh, K, T, H, W, shading=sh_name, normals=nm_name, lights=s["lights"],
                                      ambient=AMBIENT, background=BACKGROUND, znear=rc.ZNEAR, pixel_offset=off)
            assert got.shape == (1, 3, H, W) and got.dtype == torch.float32
            tag = f"{name} {W}x{H} offset {off} {sh_name}/{nm_name} (left out {left_out.mean():.4f})"
            worst = max(worst, _compare(got[0].cpu().numpy(), want["color"], keep, tag))
            worst = max(worst, _compare(got_n[0].cpu().numpy(), want["normals"], keep, tag + " normals"))
            if sh_name == "lambert":
                lit = want["color"][:, want["hit"]]
                assert ((lit > 0) & (lit < 1)).mean() > 0.5          # not a comparison of clamped values
    assert worst <= TOL


def test_thirty_two_lights_match_oracle_and_more_are_refused():
    s = _scene("room")
    sc, mesh = s["sc"], s["mesh"]
    H, W = rc.SIZES[1]
    K, T = _cams(sc, H, W)
    T0 = sc["cam_T_world"][0].astype(np.float64)
    centre = -T0[:3, :3].T @ T0[:3, 3]
    lights = [render.light_array(centre, x_length=1.0, y_length=1.0, intensity=0.05),
              render.directional_light((0.3, 0.5, 0.8), intensity=0.1)] + \
             [render.headlight(intensity=0.01 * (i + 1)) for i in range(6)]
    assert sum(len(x) for x in lights) == 32
    _, face = render.render_depth(mesh, K, T, H, W, znear=rc.ZNEAR, return_faces=True)
    got = render.render_color(mesh, K, T, H, W, lights=lights, ambient=AMBIENT, znear=rc.ZNEAR)
    want = so.shade(sc["vertices"], sc["faces"], rc.intrinsics(H, W), sc["cam_T_world"][0], H, W, 0.0,
                    face[0].cpu().numpy(), colors=s["colors"], normals=s["normals"], ambient=AMBIENT,
                    lights=np.concatenate(lights), shading=so.LAMBERT)
    keep = ~(want["hit"] & ((want["grazing"] < ro.GRAZING) | ~(want["smooth_length"] >= MIN_SMOOTH_LENGTH)))
    assert keep.mean() >= 1 - ro.MAX_CONTESTED_SHARE
    print()
    assert _compare(got[0].cpu().numpy(), want["color"], keep, "room, 32 lights") <= TOL
    with pytest.raises(ValueError):
        render.render_color(mesh, K, T, H, W, lights=lights + [render.headlight()])
    # no lights: c * ambient -- halving commutes with the rounding to fp32, so the bits are those of the unlit picture
    unlit = render.render_color(mesh, K, T, H, W, shading="unlit", znear=rc.ZNEAR)
    dark = render.render_color(mesh, K, T, H, W, shading="lambert", lights=[], ambient=0.5, znear=rc.ZNEAR)
    assert torch.equal(_bits(dark), _bits(unlit * 0.5))


def test_background_bytes_and_coverage_are_exact():
    s = _scene("junk")
    sc, mesh = s["sc"], s["mesh"]
    for (H, W), off in zip(rc.SIZES, rc.OFFSETS):       # 96 x 72: word stores; 101 x 67: an odd pixel count, two views
        K, T = _cams(sc, H, W, slice(0, 2))
        bg = (1.0, 0.0, 1.0)                             # no interpolated random colour is this
        f32, u8, depth = render.render_color(mesh, K, T, H, W, shading="unlit", background=bg, znear=rc.ZNEAR,
                                             pixel_offset=off, output="both", return_depth=True)
        assert f32.shape == (2, 3, H, W) and u8.shape == (2, H, W, 3) and u8.dtype == torch.uint8
        want_depth = render.render_depth(mesh, K, T, H, W, znear=rc.ZNEAR, pixel_offset=off)
        assert torch.equal(_bits(depth), _bits(want_depth))
        empty = (depth == 0).expand(2, 3, H, W)
        assert 0.2 < float((depth > 0).float().mean()) < 0.8
        bg_t = torch.tensor(bg, device=DEV).view(1, 3, 1, 1).expand(2, 3, H, W)
        assert torch.equal(_bits(f32[empty]), _bits(bg_t[empty]))
        is_bg = (f32 == bg_t).all(1, keepdim=True)
        assert torch.equal(is_bg, depth == 0)            # non-background exactly where the depth render hits
        assert torch.equal(u8, (f32 * 255.0).to(torch.uint8).permute(0, 2, 3, 1))
        assert float(f32.min()) >= 0.0 and float(f32.max()) <= 1.0
        only_u8 = render.render_color(mesh, K, T, H, W, shading="unlit", background=bg, znear=rc.ZNEAR, pixel_offset=off,
                                      output="u8")
        assert torch.equal(only_u8, u8)
        nrm = render.render_normals(mesh, K, T, H, W, znear=rc.ZNEAR, pixel_offset=off)
        assert bool((nrm[empty] == 0).all())
        length = nrm.norm(dim=1, keepdim=True)[depth > 0]
        assert float((length - 1).abs().max()) <= 1e-6
    # a misaligned start of the byte image (a view of odd pixel count behind another) was part of the loop above;
    # an empty mesh is all background
    none = TriangleMesh(mesh.vertices, mesh.faces[:0])
    f32, u8 = render.render_color(none, K, T, H, W, background=BACKGROUND, output="both")
    assert bool((f32 == torch.tensor(BACKGROUND, device=DEV).view(1, 3, 1, 1)).all())
    assert torch.equal(u8, (f32 * 255.0).to(torch.uint8).permute(0, 2, 3, 1))


def test_reproducible_and_batch_invariant():
    H, W = rc.SIZES[1]
    for name in ("occluder", "junk", "near"):
        s = _scene(name)
        mesh = s["mesh"]
        K, T = _cams(s["sc"], H, W, slice(0, 5))
        kw = dict(lights=s["lights"], ambient=AMBIENT, output="both")
        a = render.render_color(mesh, K, T, H, W, **kw)
        b = render.render_color(mesh, K, T, H, W, **kw)
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))
        na = render.render_normals(mesh, K, T, H, W)
        for v in range(5):
            one = render.render_color(mesh, K[v:v + 1], T[v:v + 1], H, W, **kw)
            assert all(torch.equal(_bits(x), _bits(y[v:v + 1])) for x, y in zip(one, a))
            assert torch.equal(_bits(render.render_normals(mesh, K[v:v + 1], T[v:v + 1], H, W)), _bits(na[v:v + 1]))
        plain = TriangleMesh(mesh.vertices, mesh.faces)
        assert torch.equal(_bits(render.vertex_normals(plain)), _bits(render.vertex_normals(plain)))
        assert torch.equal(_bits(render.vertex_normals(plain)), _bits(mesh.normals))


@pytest.mark.parametrize("name", rc.SCENES)
def test_vertex_normals_match_oracle(name):
    s = _scene(name)
    sc = s["sc"]
    want = so.vertex_normals(sc["vertices"], sc["faces"])
    got = s["normals"]
    assert got.shape == want.shape and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - want).max()
    zero = (want == 0).all(1)
    print(f"\n{name}: {len(want)} vertices, max abs err {err:.3e}, {int(zero.sum())} without a usable face")
    assert err <= TOL
    assert (got[zero] == 0).all()                                   # exact zeros
    assert np.abs(np.linalg.norm(got[~zero], axis=1) - 1).max() <= TOL
    if name == "junk":
        # four vertices have no usable face (zero-area or non-finite faces only), the non-finite ones among them
        assert zero.sum() == 4 and zero[~np.isfinite(sc["vertices"]).all(1)].all()
        # vertices that no face names at all, one of them non-finite, and a face with an index out of range
        more_v = torch.cat([s["mesh"].vertices, torch.tensor([[9.0, 9.0, 9.0], [np.nan, 1.0, 1.0]], device=DEV)])
        more_f = torch.cat([s["mesh"].faces, torch.tensor([[0, 1, len(want) + 2], [-1, 2, 3]], dtype=torch.int32, device=DEV)])
        more = render.vertex_normals(TriangleMesh(more_v, more_f))
        assert torch.equal(_bits(more[:-2]), _bits(s["mesh"].normals)) and bool((more[-2:] == 0).all())
    helper = render.with_vertex_normals(TriangleMesh(s["mesh"].vertices, s["mesh"].faces, None, s["mesh"].colors))
    assert torch.equal(_bits(helper.normals), _bits(s["mesh"].normals)) and helper.colors is s["mesh"].colors
    as_colors = render.normals_as_colors(s["mesh"])
    assert torch.equal(_bits(as_colors.colors), _bits((1.0 + s["mesh"].normals) / 2.0))


def _plane(n, c, extent=40.0):
    n = np.asarray(n, np.float64)
    p0 = n * c / (n @ n)
    a = np.cross(n, [0.3, 1.0, 0.1])
    a /= np.linalg.norm(a)
    b = np.cross(n, a)
    b /= np.linalg.norm(b)
    v = np.stack([p0 + extent * (sa * a + sb * b) for sa, sb in ((-1, -1), (1, -1), (1, 1), (-1, 1))])
    return v.astype(np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


def test_two_sided():
    """A plane seen from behind shades the same bits as the plane of reversed winding seen from the front."""
    H, W = rc.SIZES[1]
    v, f = _plane((0.3, -0.2, 1.0), 2.0, extent=6.0)
    colors = torch.from_numpy(np.random.default_rng(3).random((4, 3)).astype(np.float32)).to(DEV)
    K = torch.from_numpy(rc.intrinsics(H, W))[None].to(DEV)
    T = torch.eye(4, device=DEV)[None].clone()
    lights = [render.directional_light((0.2, -0.5, 1.0), intensity=0.5), render.point_light((0.5, 0.2, 0.0)),
              render.headlight(intensity=0.3)]
    pictures = {}
    for winding, faces in (("as built", f), ("reversed", f[:, [0, 2, 1]])):
        mesh = render.with_vertex_normals(TriangleMesh(torch.from_numpy(v).to(DEV),
                                                       torch.from_numpy(np.ascontiguousarray(faces)).to(DEV), None, colors))
        for cull in ("none", "back"):
            pictures[winding, cull] = render.render_color(mesh, K, T, H, W, lights=lights, ambient=AMBIENT,
                                                          background=BACKGROUND, cull=cull)
    assert torch.equal(_bits(pictures["as built", "none"]), _bits(pictures["reversed", "none"]))
    bg = torch.tensor(BACKGROUND, device=DEV).view(1, 3, 1, 1)
    culled = [w for w in ("as built", "reversed") if bool((pictures[w, "back"] == bg).all())]
    assert len(culled) == 1                                          # the one seen from behind: all background
    front = "reversed" if culled[0] == "as built" else "as built"
    assert torch.equal(_bits(pictures[front, "back"]), _bits(pictures[front, "none"]))
    assert not bool((pictures[front, "none"] == bg).all(1).any())


def test_lambert_closed_form_on_the_device():
    """The fronto-parallel quad z = 2 under one directional light: c (ambient + I max(0, n . l)) everywhere."""
    H, W = rc.SIZES[0]
    v, f = _plane((0.0, 0.0, 1.0), 2.0)
    mesh = TriangleMesh(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV))
    K = torch.from_numpy(rc.intrinsics(H, W))[None].to(DEV)
    T = torch.eye(4, device=DEV)[None].clone()
    d = np.array([0.2, -0.5, 1.0])
    inten, base = np.array([0.7, 0.5, 0.3]), np.array([0.8, 0.6, 0.4])
    cos = float(np.array([0.0, 0.0, -1.0]) @ -(d / np.linalg.norm(d)))
    want = base.astype(np.float32).astype(np.float64) * (np.float64(np.float32(0.25)) +
                                                         inten.astype(np.float32).astype(np.float64) * cos)
    for normals in ("flat", "smooth"):
        got = render.render_color(mesh, K, T, H, W, normals=normals, base_color=base, ambient=0.25,
                                  lights=render.directional_light(d, color=inten))
        err = float((got[0].double().cpu() - torch.from_numpy(want).view(3, 1, 1)).abs().max())
        print(f"\nlambert closed form, {normals}: max abs err {err:.3e}")
        assert err <= TOL
    away = render.render_color(mesh, K, T, H, W, base_color=base, ambient=0.25, lights=render.directional_light(-d))
    assert float((away[0].double().cpu() - torch.from_numpy(base * 0.25).view(3, 1, 1)).abs().max()) <= TOL


def test_renderer_wrappers():
    s = _scene("occluder")
    sc, mesh = s["sc"], s["mesh"]
    H, W = rc.SIZES[0]
    pose = np.linalg.inv(sc["cam_T_world"][0].astype(np.float64))
    K3 = rc.intrinsics(H, W)[:3, :3]
    r = render.Renderer(height=H, width=W)
    got = r.render_colour([mesh], H, W, pose, K3)
    assert isinstance(got, np.ndarray) and got.shape == (H, W, 3) and got.dtype == np.uint8
    K = torch.from_numpy(rc.intrinsics(H, W))[None].to(DEV)
    T = torch.linalg.inv(torch.from_numpy(pose)).float()[None].to(DEV)     # the camera as the Renderer forms it
    want = render.render_color(mesh, K, T, H, W, pixel_offset=0.5, cull="back", output="u8")[0].cpu().numpy()
    assert np.array_equal(got, want) and len(np.unique(got)) > 16
    # two meshes, one without colours: it gets its entry of mesh_colors
    half = len(sc["faces"]) // 2
    a = TriangleMesh(mesh.vertices, mesh.faces[:half].contiguous(), None, mesh.colors)
    b = TriangleMesh(mesh.vertices, mesh.faces[half:].contiguous())
    both = r.render_colour([a, b], H, W, pose, K3, mesh_colors=[None, (0.9, 0.2, 0.1)], cull="none")
    V = mesh.vertices.shape[0]
    joined = TriangleMesh(torch.cat([mesh.vertices, mesh.vertices]), torch.cat([mesh.faces[:half], mesh.faces[half:] + V]),
                          None, torch.cat([mesh.colors, torch.tensor((0.9, 0.2, 0.1), device=DEV).expand(V, 3)]))
    want = render.render_color(joined, K, T, H, W, pixel_offset=0.5, cull="none", output="u8")[0].cpu().numpy()
    assert np.array_equal(both, want)
    # the composite, on a mesh with faces of both orientations (the room seen from inside and its reversed copy)
    room = _scene("room")["mesh"]
    flipped = TriangleMesh(room.vertices, room.faces.flip(1).contiguous(), None, room.colors)
    pose = np.linalg.inv(_scene("room")["sc"]["cam_T_world"][0].astype(np.float64))
    kw = dict(meshes=[flipped], height=H, width=W, world_T_cam=pose, K=K3)
    culled, non_culled = r.render_colour(cull="back", **kw), r.render_colour(cull="none", **kw)
    mix = r.render_mesh_cull_composite(0.25, **kw)
    assert mix.shape == (H, W, 3) and mix.dtype == np.float64
    assert np.array_equal(mix, culled.astype(np.float64) * 0.75 + non_culled.astype(np.float64) * 0.25)
    assert not np.array_equal(culled, non_culled)


def test_example_writes_a_render(tmp_path):
    from PIL import Image
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "stream_fusion.py")
    spec = importlib.util.spec_from_file_location("stream_fusion_render", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = tmp_path / "render.png"
    predicted, _ = mod.run(frames=90, height=96, width=128, verbose=False, render_path=str(out))
    assert predicted >= 3
    picture = np.asarray(Image.open(out))
    assert picture.shape == (96, 128, 3) and picture.dtype == np.uint8
    assert (picture != 255).any()                                    # not all background
