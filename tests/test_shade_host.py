"""Host-side checks of the mesh shading: the float64 oracle (tests/shade_oracle.py) against closed forms, render.py's
argument validation and the C ABI listing (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import raster_cases as rc
import raster_oracle as ro
import shade_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("sr_mesh_vertex_normals", "sr_raster_shade")
POSE = np.eye(4)
POSE[:3, :3] = [[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]]
POSE[:3, 3] = [0.3, -0.1, 0.2]                                # a cam_T_world


def _plane_mesh(n, c, extent=40.0):
    """Two big triangles in the camera-frame plane n . X = c."""
    n = np.asarray(n, np.float64)
    p0 = n * c / (n @ n)
    a = np.cross(n, [0.3, 1.0, 0.1])
    a /= np.linalg.norm(a)
    b = np.cross(n, a)
    b /= np.linalg.norm(b)
    v = np.stack([p0 + extent * (sa * a + sb * b) for sa, sb in ((-1, -1), (1, -1), (1, 1), (-1, 1))])
    return v, np.array([[0, 1, 2], [0, 2, 3]])


def _to_world(v_cam, T):
    return (v_cam - T[:3, 3]) @ T[:3, :3]                     # world = R^T (cam - t)


@pytest.mark.parametrize("off", rc.OFFSETS)
def test_oracle_unlit_quad_is_affine_in_the_pixel(off):
    H, W = 37, 51
    K = rc.intrinsics(H, W).astype(np.float64)
    z = 2.0
    v = np.array([[-0.5, -0.4, z], [0.6, -0.4, z], [0.6, 0.3, z], [-0.5, 0.3, z]])
    f = np.array([[0, 1, 2], [0, 2, 3]])
    A = np.array([[0.3, 0.1], [-0.2, 0.4], [0.1, -0.3]])
    b = np.array([0.5, 0.4, 0.6])
    colors = v[:, :2] @ A.T + b                               # corner colours of one affine function of (x, y)
    assert colors.min() > 0.05 and colors.max() < 0.95
    face = ro.cast(v, f, K, np.eye(4), H, W, 0.05, off)["face"]
    assert (face >= 0).any() and (face < 0).any() and {0, 1} <= set(np.unique(face))
    r = so.shade(v, f, K, np.eye(4), H, W, off, face, colors=colors, shading=so.UNLIT, background=(1.0, 0.0, 1.0))
    yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    xy = np.stack([z * (xx + off - K[0, 2]) / K[0, 0], z * (yy + off - K[1, 2]) / K[1, 1]], -1)
    want = np.moveaxis(xy @ A.T + b, -1, 0)
    hit = face >= 0
    assert np.array_equal(r["hit"], hit)
    assert np.abs(r["color"] - want)[:, hit].max() <= 1e-12
    assert (r["color"][:, ~hit] == np.array([1.0, 0.0, 1.0])[:, None]).all()
    assert (r["normals"][:, ~hit] == 0).all()
    assert np.abs(r["normals"][:, hit] - np.array([0.0, 0.0, -1.0])[:, None]).max() <= 1e-12   # faces the viewer


@pytest.mark.parametrize("off", rc.OFFSETS)
def test_oracle_interpolation_is_perspective_correct(off):
    H, W = 37, 51
    K = rc.intrinsics(H, W).astype(np.float64)
    n, c = np.array([0.3, -0.2, 1.0]), 2.0
    v_cam, f = _plane_mesh(n, c, extent=6.0)
    vw = _to_world(v_cam, POSE)
    G = np.array([[0.02, -0.01, 0.015], [-0.015, 0.02, 0.01], [0.01, 0.01, -0.02]])
    g0 = np.array([0.5, 0.45, 0.55])
    attr = vw @ G.T + g0                                      # linear in the world position
    assert attr.min() > 0.05 and attr.max() < 0.95
    face = ro.cast(vw, f, K, POSE, H, W, 0.05, off)["face"]
    assert (face >= 0).all()
    r = so.shade(vw, f, K, POSE, H, W, off, face, colors=attr, shading=so.UNLIT)
    P = r["point"]
    assert np.abs(P @ n - c).max() <= 1e-12                   # the hit point lies in the plane ...
    rays = ro.rays(K, H, W, off).reshape(H, W, 3)
    assert np.abs(np.cross(P, rays)).max() <= 1e-12           # ... and on the pixel's ray
    want = _to_world(P, POSE) @ G.T + g0                      # the function at the hit point
    assert np.abs(np.moveaxis(r["color"], 0, -1) - want).max() <= 1e-12
    assert np.abs(r["weights"].sum(-1) - 1).max() <= 1e-12 and r["weights"].min() >= 0


@pytest.mark.parametrize("mode", (so.FLAT, so.SMOOTH))
def test_oracle_lambert_on_a_plane(mode):
    H, W = 24, 32
    K = rc.intrinsics(H, W).astype(np.float64)
    n, c = np.array([0.3, -0.2, 1.0]), 2.0
    v_cam, f = _plane_mesh(n, c)
    vw = _to_world(v_cam, POSE)
    face = ro.cast(vw, f, K, POSE, H, W, 0.05, 0.0)["face"]
    d_world = np.array([0.2, -0.5, 1.0])
    inten = np.array([0.7, 0.5, 0.3])
    light = np.array([[so.DIRECTIONAL, *d_world, *inten, 0.0]])
    base = np.array([0.8, 0.6, 0.4])
    normals = so.vertex_normals(vw, f)
    r = so.shade(vw, f, K, POSE, H, W, 0.0, face, normals=normals, base_color=base, ambient=0.25, lights=light,
                 shading=so.LAMBERT, normal_mode=mode)
    n_view = -n / np.linalg.norm(n)                           # the plane is in front: its normal towards the camera
    ell = -(POSE[:3, :3] @ (d_world / np.linalg.norm(d_world)))
    cos = max(0.0, float(n_view @ ell))
    assert cos > 0.1
    want = base * (0.25 + inten * cos)
    assert np.abs(r["color"] - want[:, None, None]).max() <= 1e-12
    assert np.abs(r["normals"] - n_view[:, None, None]).max() <= 1e-12
    # seen from behind (reversed winding: the same surface, back-facing): the same picture
    r2 = so.shade(vw, f[:, ::-1], K, POSE, H, W, 0.0, face, normals=so.vertex_normals(vw, f[:, ::-1]), base_color=base,
                  ambient=0.25, lights=light, shading=so.LAMBERT, normal_mode=mode)
    assert np.abs(r2["color"] - r["color"]).max() <= 1e-12
    # no lights: c * ambient; a light behind the surface adds nothing
    r3 = so.shade(vw, f, K, POSE, H, W, 0.0, face, base_color=base, ambient=0.25, shading=so.LAMBERT)
    assert np.abs(r3["color"] - (base * 0.25)[:, None, None]).max() <= 1e-15
    away = np.array([[so.DIRECTIONAL, *(-d_world), *inten, 0.0]])
    r4 = so.shade(vw, f, K, POSE, H, W, 0.0, face, base_color=base, ambient=0.25, lights=away, shading=so.LAMBERT)
    assert np.abs(r4["color"] - (base * 0.25)[:, None, None]).max() <= 1e-15


def test_oracle_point_and_head_lights():
    """One pixel by hand: the plane z = 2, the pixel on the optical axis."""
    H = W = 1
    K = np.eye(4)
    K[0, 0] = K[1, 1] = 10.0
    v, f = _plane_mesh((0.0, 0.0, 1.0), 2.0)
    face = np.zeros((1, 1), np.int64)
    base = np.array([1.0, 0.5, 0.25])
    lights = np.array([[so.POINT, 1.5, 0.0, 0.0, 0.8, 0.8, 0.8, 0.0], [so.HEAD, 0.0, 0.0, 0.0, 0.1, 0.2, 0.3, 0.0]])
    r = so.shade(v, f, K, np.eye(4), H, W, 0.0, face, base_color=base, ambient=0.0, lights=lights, shading=so.LAMBERT)
    # P = (0, 0, 2), n = (0, 0, -1); point light at distance 2.5 with cosine 2 / 2.5; headlight cosine 1
    want = base * (0.8 * (2.0 / 2.5) / 6.25 + np.array([0.1, 0.2, 0.3]))
    assert np.abs(r["color"][:, 0, 0] - want).max() <= 1e-15
    rn = so.shade(v, f, K, np.eye(4), H, W, 0.0, face, shading=so.NORMALS)
    assert np.abs(rn["color"][:, 0, 0] - np.array([0.5, 0.5, 0.0])).max() <= 1e-15


def _sphere(levels=3):
    """A subdivided octahedron projected to the unit sphere, wound counter-clockwise seen from outside."""
    v = [np.array(p, np.float64) for p in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1))]
    f = [(0, 2, 4), (2, 1, 4), (1, 3, 4), (3, 0, 4), (2, 0, 5), (1, 2, 5), (3, 1, 5), (0, 3, 5)]
    for _ in range(levels):
        mid, nf = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                p = v[i] + v[j]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
        f = nf
    v, f = np.stack(v), np.array(f)
    out = (np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]) * v[f].mean(1)).sum(1)
    assert (out > 0).all()
    return v, f


def test_oracle_vertex_normals():
    v, f = _sphere()
    assert len(f) == 512
    n = so.vertex_normals(v.astype(np.float32), f)
    tri = v[f]
    face_angle = max(np.arccos(np.clip((tri[:, i] * tri[:, j]).sum(1), -1, 1)).max() for i, j in ((0, 1), (1, 2), (2, 0)))
    angle = np.arccos(np.clip((n * v).sum(1), -1, 1))
    print(f"\nsphere: largest face angle {face_angle:.4f} rad, largest normal deviation {angle.max():.4f} rad")
    assert angle.max() <= face_angle
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 1e-12
    # an isolated vertex gives zero; a face with a NaN vertex, or an index out of range, is skipped
    v2 = np.concatenate([v, [[5.0, 5.0, 5.0], [np.nan, 0.0, 0.0]]]).astype(np.float32)
    f2 = np.concatenate([f, [[0, 1, len(v) + 1], [2, 3, len(v) + 7], [4, -1, 5]]])
    n2 = so.vertex_normals(v2, f2)
    assert np.array_equal(n2[:len(v)], n)
    assert (n2[len(v):] == 0).all()
    # area weighting: a large and a small face at one vertex
    v3 = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0], [0, 0, 1], [0, 1, 0]], np.float64)
    f3 = np.array([[0, 1, 2], [0, 3, 4]])
    want = np.array([0.0, 0.0, 16.0]) + np.array([-1.0, 0.0, 0.0])
    assert np.abs(so.vertex_normals(v3, f3)[0] - want / np.linalg.norm(want)).max() <= 1e-15


@pytest.mark.parametrize("name", rc.SCENES)
def test_stored_scenes_stay_under_the_left_out_cap(name):
    """What the GPU comparison leaves out -- grazing winners and pixels whose interpolated normal nearly cancels -- on
    the oracle's own face image: at most 3 % of a picture (measured when this was written: none, on every case)."""
    sc = rc.load(name)
    normals = so.vertex_normals(sc["vertices"], sc["faces"])
    for H, W in rc.SIZES:
        for off in rc.OFFSETS:
            K = rc.intrinsics(H, W)
            face = ro.cast(sc["vertices"], sc["faces"], K, sc["cam_T_world"][0], H, W, rc.ZNEAR, off)["face"]
            r = so.shade(sc["vertices"], sc["faces"], K, sc["cam_T_world"][0], H, W, off, face, normals=normals,
                         shading=so.NORMALS)
            grazing = r["hit"] & (r["grazing"] < ro.GRAZING)
            short = r["hit"] & ~(r["smooth_length"] >= 0.05)
            print(f"{name} {W}x{H} offset {off}: grazing {grazing.mean():.4f}, short normal {short.mean():.4f}")
            assert (grazing | short).mean() <= ro.MAX_CONTESTED_SHARE
            assert np.abs(np.linalg.norm(r["normals"], axis=0) - 1)[r["hit"]].max() <= 1e-12


def _host_mesh():
    from simplerecon_amd.tsdf import TriangleMesh
    v = torch.tensor([[0.0, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]])
    f = torch.tensor([[0, 1, 2]], dtype=torch.int32)
    return TriangleMesh(v, f), v, f


def test_render_color_validation():
    from simplerecon_amd import render
    from simplerecon_amd._lib import HipLibraryError
    from simplerecon_amd.tsdf import TriangleMesh
    mesh, v, f = _host_mesh()
    K = torch.from_numpy(rc.intrinsics(8, 12))[None]
    T = torch.eye(4)[None]
    for fn in (render.render_color, render.render_normals):
        with pytest.raises(HipLibraryError):
            fn(mesh, K, T, 8, 12)                                    # host tensors: no CPU fallback
        with pytest.raises(ValueError):
            fn(mesh, K, T, 8, 12, normals="bumpy")
        with pytest.raises(ValueError):
            fn(mesh, K, T, 8, 12, cull="front-ish")
        with pytest.raises(ValueError):
            fn(mesh, K, T, 0, 12)
        with pytest.raises(ValueError):
            fn(mesh, K, T, 8, 12, znear=0.0)
        with pytest.raises(ValueError):
            fn(mesh, K, T, 8, 12, pixel_offset=2.0)
        with pytest.raises(TypeError):
            fn((v, f), K, T, 8, 12)
        with pytest.raises(TypeError):
            fn(TriangleMesh(v.double(), f), K, T, 8, 12)
        with pytest.raises(ValueError):
            fn(TriangleMesh(v[:, :2], f), K, T, 8, 12)
    for bad in (dict(shading="phong"), dict(output="f16"), dict(ambient=-0.1), dict(ambient=float("nan")),
                dict(base_color=(0.5, 0.5)), dict(base_color=(0.5, 0.5, 1.5)), dict(background=(0.0, 0.0, float("inf"))),
                dict(lights=np.zeros((33, 8), np.float32)), dict(lights=[render.light_array((0, 0, 0)), render.light_array((0, 0, 1))]),
                dict(lights=np.zeros((2, 7), np.float32)), dict(lights=np.array([[3, 0, 0, 1, 1, 1, 1, 0]], np.float32)),
                dict(lights=np.array([[0.5, 0, 0, 1, 1, 1, 1, 0]], np.float32)),
                dict(lights=np.array([[1, 0, np.nan, 1, 1, 1, 1, 0]], np.float32))):
        with pytest.raises(ValueError):
            render.render_color(mesh, K, T, 8, 12, **bad)
    with pytest.raises(TypeError):
        render.render_color(mesh, K, T, 8, 12, lights=[object()])
    # 32 lights pass the light check (the host mesh is what is refused then)
    with pytest.raises(HipLibraryError):
        render.render_color(mesh, K, T, 8, 12, lights=np.zeros((32, 8), np.float32))
    # colours and normals: [V,3] fp32 on the mesh's device
    with pytest.raises(ValueError):
        render._check_attribute("mesh.colors", torch.zeros(4, 3), v)
    with pytest.raises(TypeError):
        render._check_attribute("mesh.colors", torch.zeros(3, 3, dtype=torch.float64), v)
    with pytest.raises(TypeError):
        render._check_attribute("mesh.normals", np.zeros((3, 3), np.float32), v)
    with pytest.raises(HipLibraryError):
        render._check_attribute("mesh.normals", torch.zeros(3, 3), v)
    assert render._check_attribute("mesh.colors", None, v) is None
    assert render.SHADING_MODES == {"unlit": 0, "normals": 1, "lambert": 2}
    assert render.NORMAL_MODES == {"smooth": 0, "flat": 1}
    assert render.LIGHT_KINDS == {"directional": 0, "point": 1, "headlight": 2}
    assert render.MAX_LIGHTS == 32 and render.LIGHT_FLOATS == 8


def test_vertex_normals_validation():
    from simplerecon_amd import render
    from simplerecon_amd._lib import HipLibraryError
    from simplerecon_amd.tsdf import TriangleMesh
    mesh, v, f = _host_mesh()
    for fn in (render.vertex_normals, render.with_vertex_normals, render.normals_as_colors):
        with pytest.raises(HipLibraryError):
            fn(mesh)
        with pytest.raises(TypeError):
            fn((v, f))
        with pytest.raises(TypeError):
            fn(TriangleMesh(v, f.long()))
        with pytest.raises(ValueError):
            fn(TriangleMesh(v, f.reshape(3, 1)))


def test_light_helpers():
    from simplerecon_amd import render
    d = render.directional_light((0.0, 0.0, 2.0), color=(1.0, 0.5, 0.25), intensity=2.0)
    assert d.shape == (1, 8) and d.dtype == np.float32
    assert np.array_equal(d[0], np.array([0, 0, 0, 2, 2.0, 1.0, 0.5, 0], np.float32))
    p = render.point_light(torch.tensor([1.0, 2.0, 3.0]))
    assert np.array_equal(p[0], np.array([1, 1, 2, 3, 1, 1, 1, 0], np.float32))
    h = render.headlight(intensity=0.6)
    assert np.array_equal(h[0], np.array([2, 0, 0, 0, 0.6, 0.6, 0.6, 0], np.float32))
    g = render.light_array((1.0, 2.0, 3.0))
    assert g.shape == (25, 8) and (g[:, 0] == 1).all() and (g[:, 3] == 3).all() and (g[:, 4:7] == 1).all()
    assert np.array_equal(np.unique(g[:, 1]), 1 + np.linspace(-10, 10, 5).astype(np.float32))
    assert np.array_equal(np.unique(g[:, 2]), 2 + np.linspace(-10, 10, 5).astype(np.float32))
    assert len({(x, y) for x, y in g[:, 1:3]}) == 25
    g = render.light_array((0, 0, 0), x_length=1.0, y_length=2.0, num_x=3, num_y=2, intensity=0.5)
    assert g.shape == (6, 8) and set(g[:, 1]) == {-1.0, 0.0, 1.0} and set(g[:, 2]) == {-2.0, 2.0} and (g[:, 4] == 0.5).all()
    both = render._check_lights([d, p, h])
    assert both.shape == (3, 8) and list(both[:, 0]) == [0, 1, 2]
    assert np.array_equal(render._check_lights(None), render.headlight(intensity=0.6))
    assert render._check_lights([]).shape == (0, 8)
    for bad in (lambda: render.directional_light((0.0, 0.0, 0.0)), lambda: render.directional_light((1.0, 2.0)),
                lambda: render.point_light((1.0, float("nan"), 0.0)), lambda: render.headlight(intensity=-1.0),
                lambda: render.headlight(color=(1.0, -1.0, 0.0)), lambda: render.light_array((0, 0, 0), num_x=0),
                lambda: render.light_array((0, 0), num_x=2)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        render.point_light("here")


def test_renderer_validation():
    from simplerecon_amd import render
    mesh, v, f = _host_mesh()
    r = render.Renderer(8, 12)
    with pytest.raises(NotImplementedError):
        r.render_mesh([mesh], 8, 12, np.eye(4), np.eye(3), get_colour=True)
    with pytest.raises(TypeError):
        r.render_colour([], 8, 12, np.eye(4), np.eye(3))
    with pytest.raises(TypeError):
        r.render_colour([mesh, (v, f)], 8, 12, np.eye(4), np.eye(3))
    with pytest.raises(ValueError):
        r.render_colour([mesh], 8, 12, np.eye(4), np.eye(3), mesh_colors=[(1, 0, 0), (0, 1, 0)])
    with pytest.raises(ValueError):
        r.render_colour([mesh], 8, 12, np.eye(4), np.eye(3), mesh_colors=[(2.0, 0, 0)])
    with pytest.raises(ValueError):
        r.render_colour([mesh], 8, 12, np.eye(4), np.eye(3), cull="front-ish")
    with pytest.raises(ValueError):
        r.render_colour([mesh], 8, 12, np.eye(4), np.eye(3), lights=np.zeros((33, 8), np.float32))
    with pytest.raises(TypeError):
        r.render_mesh_cull_composite(0.25, meshes=[mesh], height=8, width=12, world_T_cam=np.eye(4), K=np.eye(3),
                                     cull="back")


def test_symbols_are_declared_bound_and_exported():
    from simplerecon_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "simplerecon_hip.h")).read()
    assert re.search(r"-+ mesh rasteriser -+.*-+ mesh shading -+.*-+ frame preparation -+", hdr, flags=re.S)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in the header"
        assert name in _lib.SIGNATURES and hasattr(raw, name)
        getattr(raw, name).restype, getattr(raw, name).argtypes = _lib.SIGNATURES[name]
    assert _lib.ABI_VERSION == 5 and raw.sr_abi_version() == 5
    for macro, value in (("SR_SHADE_UNLIT", 0), ("SR_SHADE_NORMALS", 1), ("SR_SHADE_LAMBERT", 2),
                         ("SR_SHADE_NORMAL_SMOOTH", 0), ("SR_SHADE_NORMAL_FLAT", 1), ("SR_SHADE_LIGHT_DIRECTIONAL", 0),
                         ("SR_SHADE_LIGHT_POINT", 1), ("SR_SHADE_LIGHT_HEAD", 2), ("SR_SHADE_MAX_LIGHTS", 32),
                         ("SR_SHADE_LIGHT_FLOATS", 8)):
        assert re.search(rf"#define {macro} {value}\b", hdr)

    # host-side refusals of the entry points: every one of these returns before any launch
    buf = (ctypes.c_float * 16)()                  # stands in for device arrays, which the host never reads
    dev = ctypes.addressof(buf)
    assert raw.sr_mesh_vertex_normals(None, 4, None, 4, None, None, None, None) == 1
    assert raw.sr_mesh_vertex_normals(dev, 4, dev, 4, dev, dev, None, None) == 1
    assert raw.sr_mesh_vertex_normals(dev, 0, dev, 4, dev, dev, dev, None) == 1
    rgb = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    lights = (ctypes.c_float * (33 * 8))()

    def shade(**kw):
        a = dict(vertices=dev, V=4, faces=dev, F=4, K=dev, T=dev, B=1, H=8, W=12, off=0.0, face=dev, colors=None,
                 normals=None, base=ctypes.addressof(rgb), bg=ctypes.addressof(rgb), ambient=0.4,
                 lights=ctypes.addressof(lights), num_lights=1, shading=2, normal_mode=0, out_f32=dev, out_u8=None,
                 normals_out=None)
        assert set(kw) <= set(a)
        a.update(kw)
        return raw.sr_raster_shade(*a.values(), None)

    for kw in (dict(vertices=None), dict(faces=None), dict(K=None), dict(T=None), dict(face=None), dict(base=None),
               dict(bg=None), dict(out_f32=None), dict(lights=None), dict(num_lights=33), dict(num_lights=-1),
               dict(shading=3), dict(shading=-1), dict(normal_mode=2), dict(H=32769), dict(W=0), dict(B=0),
               dict(B=70000, H=256, W=256), dict(off=1.5), dict(V=0), dict(F=0)):
        assert shade(**kw) == 1, kw
    lights[8] = 3.0                                # the second light's kind
    assert shade(num_lights=2) == 1
    lights[8] = 0.5
    assert shade(num_lights=2) == 1
