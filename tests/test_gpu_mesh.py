"""GPU marching cubes (csrc/sr_mesh.hip via TSDF.extract_mesh): agreement with the numpy rules of tests/mesh_oracle.py,
oracle-free surface invariants, exact zeros, fused volumes and refusals."""
import time

import numpy as np
import pytest
import torch

import mesh_oracle as mo
import tsdf_cases
from simplerecon_amd import _lib
from simplerecon_amd.tsdf import TSDF, OurFuser, marching_cubes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _grid(shape, center):
    g = np.stack(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"), -1).astype(np.float64)
    return g - np.asarray(center, dtype=np.float64)


def sphere(shape, R, center):
    return ((np.linalg.norm(_grid(shape, center), axis=-1) - R) / 4.0).astype(np.float16)


def torus(shape, Rm, r, center):
    g = _grid(shape, center)
    q = np.sqrt(g[..., 0] ** 2 + g[..., 1] ** 2) - Rm
    return ((np.sqrt(q ** 2 + g[..., 2] ** 2) - r) / 4.0).astype(np.float16)


def noise(shape, seed, smooth=3.0, amp=0.8):
    """Gaussian-filtered white noise (periodic), scaled so that much of it lies inside [-1, 1]."""
    r = np.random.default_rng(seed).standard_normal(shape)
    k = np.meshgrid(*[np.fft.fftfreq(s) for s in shape], indexing="ij")
    k2 = sum(x ** 2 for x in k)
    out = np.real(np.fft.ifftn(np.fft.fftn(r) * np.exp(-k2 * (2 * np.pi * smooth) ** 2 / 2)))
    return (out / out.std() * amp).astype(np.float16)


def _gpu(vol, normals=True):
    m = marching_cubes(torch.from_numpy(vol).to(DEV), compute_normals=normals)
    torch.cuda.synchronize()
    return (m.vertices.cpu().numpy(), m.faces.cpu().numpy(), None if m.normals is None else m.normals.cpu().numpy())


def _closed_check(faces):
    f = faces.astype(np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    s = set(map(tuple, d.tolist()))
    assert len(s) == len(d), "a directed edge is used twice"
    assert all((b, a) in s for a, b in s), "an edge is not shared by two faces with opposite directions"
    return len(np.unique(f)) - len(s) // 2 + len(f)   # Euler characteristic


def _volume(v, f):
    a, b, c = (v[f[:, i]].astype(np.float64) for i in range(3))
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def _assert_matches_oracle(vol):
    v, f, n = _gpu(vol)
    vo, fo, no, _ = mo.marching_cubes(vol)
    assert v.shape == vo.shape and f.shape == fo.shape
    assert np.abs(v - vo).max(initial=0.0) <= 1e-6 * max(1.0, float(np.abs(vo).max(initial=0.0)))
    assert np.array_equal(mo.canonical_faces(f), mo.canonical_faces(fo))
    assert np.abs(n - no).max(initial=0.0) < 1e-5
    return v, f, n


CASES = {
    "sphere32": lambda: sphere((32, 32, 32), 11.0, (15.7, 15.2, 16.1)),
    "sphere_odd": lambda: sphere((21, 18, 27), 7.3, (10.1, 8.6, 13.2)),
    "torus48": lambda: torus((48, 48, 40), 14.0, 5.5, (23.6, 23.3, 19.8)),
    "noise64": lambda: noise((64, 64, 64), 1, smooth=1.5),
    "noise_odd": lambda: noise((37, 23, 19), 2, smooth=2.0),
    "noise_ambiguous": lambda: noise((24, 16, 40), 3, smooth=0.7, amp=1.5),
}


@pytest.mark.parametrize("name", list(CASES))
def test_mesh_matches_oracle(name):
    vol = CASES[name]()
    _, f, _ = _assert_matches_oracle(vol)
    assert len(f) > 0


@pytest.mark.parametrize("shape, nbricks, chunk, busy", [((160, 168, 128), 1680, 2, 840), ((200, 200, 160), 3125, 4, 782)])
def test_mesh_matches_oracle_past_1024_bricks(shape, nbricks, chunk, busy):
    """More bricks than sr_mesh_scan_kernel has threads: every thread sums and offsets `chunk` > 1 bricks, and with chunk 4
    the threads from 782 on have none (tsdf_cases.mesh_plan restates the arithmetic)."""
    plan = tsdf_cases.mesh_plan(shape)
    assert (plan["nbricks"], plan["chunk"], plan["busy_threads"]) == (nbricks, chunk, busy) and busy < 1024 < nbricks
    _, f, _ = _assert_matches_oracle(noise(shape, 11, smooth=6))
    assert len(f) > 1000


def test_ambiguous_faces_are_exercised():
    """The noise case has many cube faces where the asymptotic decider chooses."""
    v = np.clip(CASES["noise_ambiguous"]().astype(np.float32), -1, 1)
    up = ~(v < 0)
    n_amb = 0
    for a in range(3):
        s = [slice(None)] * 3
        def sl(d0, d1):
            t = list(s)
            o = [x for x in range(3) if x != a]
            t[o[0]] = slice(d0, v.shape[o[0]] - 1 + d0)
            t[o[1]] = slice(d1, v.shape[o[1]] - 1 + d1)
            return up[tuple(t)]
        p00, p10, p11, p01 = sl(0, 0), sl(1, 0), sl(1, 1), sl(0, 1)
        n_amb += int(((p00 == p11) & (p10 == p01) & (p00 != p10)).sum())
    assert n_amb > 200


def test_sphere_invariants():
    R, c = 20.0, (24.3, 23.8, 24.6)
    vol = sphere((50, 48, 49), R, c)
    m = marching_cubes(torch.from_numpy(vol).to(DEV))
    v, f, n = m.vertices.cpu().numpy(), m.faces.cpu().numpy(), m.normals.cpu().numpy()
    assert _closed_check(f) == 2
    V = _volume(v, f)
    assert V > 0 and abs(V / (4.0 / 3.0 * np.pi * R ** 3) - 1.0) < 0.01
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    grad = v[f].mean(1) - np.asarray(c)                       # analytic gradient of |x - c|
    assert (np.einsum("ij,ij->i", fn, grad) > 0).all()
    assert (np.einsum("ij,ij->i", n, v - np.asarray(c)) > 0).all()
    assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-5)


def test_torus_invariants():
    c = (31.4, 32.2, 15.7)
    vol = torus((64, 64, 32), 18.0, 7.0, c)
    v, f, _ = _gpu(vol, normals=False)
    assert _closed_check(f) == 0
    assert _volume(v, f) > 0
    g = v[f].mean(1) - np.asarray(c)
    rho = np.sqrt(g[:, 0] ** 2 + g[:, 1] ** 2)
    grad = np.stack([g[:, 0] * (1 - 18.0 / rho), g[:, 1] * (1 - 18.0 / rho), g[:, 2]], 1)
    fn = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    assert (np.einsum("ij,ij->i", fn, grad) > 0).all()


@pytest.mark.parametrize("seed", [4, 5])
def test_noise_open_edges_lie_on_the_volume_boundary(seed):
    shape = (33, 40, 24)
    vol = noise(shape, seed, smooth=1.2)
    v, f, _ = _gpu(vol, normals=False)
    f = f.astype(np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und = np.sort(d, 1)
    uniq, inv, cnt = np.unique(und, axis=0, return_inverse=True, return_counts=True)
    # a shared edge is used as often in one direction as in the other (a fan diagonal across an ambiguous cube face
    # can be shared by the two cubes of that face: 4 uses)
    fwd = np.bincount(inv.reshape(-1), weights=(d[:, 0] < d[:, 1]), minlength=len(uniq))
    assert np.array_equal(2 * fwd[cnt > 1], cnt[cnt > 1])
    once = uniq[cnt == 1]
    assert len(once) > 0
    pa, pb = v[once[:, 0]], v[once[:, 1]]
    hi = np.asarray(shape, dtype=np.float32) - 1
    on_face = ((pa == 0) & (pb == 0)) | ((pa == hi) & (pb == hi))
    assert on_face.any(1).all()


@pytest.mark.parametrize("step", [0.5, 0.25])
def test_exact_zeros_give_no_degenerate_triangles(step):
    base = noise((30, 26, 32), 7, smooth=1.5).astype(np.float32)
    vol = (np.round(base / step) * step).astype(np.float16)
    assert int((vol == 0).sum()) > 500
    v, f, _ = _assert_matches_oracle(vol)
    p = v[f]
    for i, j in ((0, 1), (1, 2), (0, 2)):
        assert not (p[:, i] == p[:, j]).all(1).any()
    assert len(np.unique(f)) <= len(v)


def test_scalar_path_matches_vector_path():
    """Z % 8 == 0 takes 16-byte loads; an offset view of the same values takes the scalar path."""
    vol = noise((20, 24, 32), 9, smooth=1.5)
    a = marching_cubes(torch.from_numpy(vol).to(DEV))
    buf = torch.empty(vol.size + 1, dtype=torch.float16, device=DEV)
    buf[1:] = torch.from_numpy(vol).reshape(-1).to(DEV)
    b = marching_cubes(buf[1:].view(vol.shape))
    assert torch.equal(a.vertices, b.vertices) and torch.equal(a.faces, b.faces) and torch.equal(a.normals, b.normals)


def _room(fuser, frames=4, seed=3, near=1.0, span=1.5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    depth = (near + span * torch.rand((frames, 1, 48, 64), generator=g))
    depth = torch.nn.functional.interpolate(depth, size=(480, 640), mode="bilinear", align_corners=False)
    K = torch.eye(4).repeat(frames, 1, 1)
    K[:, 0, 0] = K[:, 1, 1] = 577.87
    K[:, 0, 2], K[:, 1, 2] = 320.0, 240.0
    T = torch.eye(4).repeat(frames, 1, 1)
    for i in range(frames):
        T[i, 0, 3] = 0.05 * i
    fuser.fuse_frames(depth.to(DEV), K.to(DEV), T.to(DEV), None)


def test_fused_room_mesh():
    bounds = dict(xmin=-3.2, xmax=3.2, ymin=-3.2, ymax=3.2, zmin=0.0, zmax=3.2)
    fuser = OurFuser(bounds=bounds, max_fusion_depth=3.0, device=DEV)
    _room(fuser)
    a = fuser.get_mesh()
    b = fuser.tsdf_fuser_pred.tsdf.extract_mesh()
    assert a.faces.shape[0] > 1000
    assert torch.equal(a.vertices.view(torch.int32), b.vertices.view(torch.int32))
    assert torch.equal(a.faces, b.faces) and torch.equal(a.normals.view(torch.int32), b.normals.view(torch.int32))
    v, f = a.vertices.cpu().numpy(), a.faces.cpu().numpy()
    vol = fuser.tsdf_fuser_pred.tsdf
    o = vol.origin.float().numpy()
    hi = o + (np.asarray(vol.tsdf_values.shape) - 1) * vol.voxel_size
    assert (v >= o - 1e-4).all() and (v <= hi + 1e-4).all()
    assert f.min() >= 0 and f.max() < len(v)
    # world coordinates are fp16 origin + voxel units * voxel size
    u = vol.extract_mesh(scale_to_world=False, compute_normals=False)
    assert u.normals is None
    w = o[None] + u.vertices.cpu().numpy() * np.float32(vol.voxel_size)
    assert np.array_equal(w, v)


def test_default_volume_mesh():
    """The default 504^3 volume (62 512 bricks: every thread of the scan owns 62) against the oracle on a crop.

    The fused surface is a close one (depths 0.2 .. 0.35 m), because the box of touched voxels is wide whatever the depth: the
    voxel layers next to the camera plane are updated out to the volume's faces (their fp16 pixel coordinates overflow and the
    fuser samples texel 0, as the reference does), so the box spans all of x and y and only its z extent -- the sheet's few
    layers plus depth + truncation -- can be kept small enough for the oracle (at most 4 M voxels).  That sheet also puts
    active bricks all along the brick order, which is what the scan's offsets need.

    Outside the box every voxel is -1, so no edge out there crosses the level, and both sides walk voxels lexicographically:
    the crop's mesh is the volume's mesh with vertex coordinates shifted by the crop's offset, vertex for vertex and face for
    face.  Dilating the box by 2 voxels gives the normals' central differences the same neighbours on both sides."""
    fuser = OurFuser(max_fusion_depth=3.0, device=DEV)
    assert tuple(fuser.tsdf_fuser_pred.shape) == (504, 504, 504)
    assert tsdf_cases.mesh_plan((504, 504, 504))["chunk"] == 62
    _room(fuser, frames=2, near=0.2, span=0.15)
    torch.cuda.synchronize()
    t0 = time.monotonic()
    m = fuser.get_mesh()
    torch.cuda.synchronize()
    dt = time.monotonic() - t0
    assert m.faces.shape[0] > 1000 and m.vertices.shape[0] > 1000
    assert int(m.faces.min()) >= 0 and int(m.faces.max()) < m.vertices.shape[0]
    assert dt < 30.0, f"504^3 extraction took {dt:.1f} s"

    vol = fuser.tsdf_fuser_pred.tsdf
    touched = vol.tsdf_weights > 0
    lo, hi = [], []
    for a in range(3):
        idx = torch.nonzero(touched.any(dim=tuple(d for d in range(3) if d != a)))[:, 0]
        lo.append(max(0, int(idx.min()) - 2))
        hi.append(min(504, int(idx.max()) + 1 + 2))
    size = (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2])
    print(f"box of touched voxels, dilated by 2: {lo} .. {hi}, {size} voxels")
    assert size <= 4_000_000, f"the dilated box {lo} .. {hi} is too large for the oracle"
    unchanged = vol.tsdf_values == -1
    unchanged[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = True
    assert bool(unchanged.all()), "a voxel outside the box is not -1"
    del unchanged, touched
    crop = vol.tsdf_values[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]].cpu().numpy()
    vo, fo, no, _ = mo.marching_cubes(crop)
    u = vol.extract_mesh(scale_to_world=False)
    v, f, n = u.vertices.cpu().numpy(), u.faces.cpu().numpy(), u.normals.cpu().numpy()
    assert len(v) == len(vo) == m.vertices.shape[0] and f.shape == fo.shape == tuple(m.faces.shape)
    assert np.array_equal(f, fo), "faces differ from the crop's, or come in another order"
    assert np.abs(n - no).max(initial=0.0) < 1e-5
    # A coordinate is index + t in fp32, t in [0, 1) the crossing's position on its edge.  Index + t < 512, where fp32 values are
    # 2^-15 apart: the volume's mesh rounds it once (error <= 2^-16); the crop's mesh rounds (index - lo) + t, also below 512,
    # once (<= 2^-16), and the offset is added here in float64 (exact).  t itself is the same fp32 expression on both sides,
    # allowed one unit in its last place (2^-23, the spacing just below 1) as in _assert_matches_oracle.
    bound = 2.0 ** -16 + 2.0 ** -16 + 2.0 ** -23
    err = float(np.abs(v.astype(np.float64) - (vo.astype(np.float64) + np.asarray(lo, np.float64))).max())
    print(f"vertex error {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_save_and_export(tmp_path):
    fuser = OurFuser(bounds=dict(xmin=-1.0, xmax=1.0, ymin=-1.0, ymax=1.0, zmin=0.0, zmax=2.56), device=DEV)
    _room(fuser, frames=1)
    ref = fuser.get_mesh().cpu()
    fuser.export_mesh(str(tmp_path / "m.ply"))
    with pytest.raises(ValueError):
        fuser.export_mesh(str(tmp_path / "m.obj"))
    vol = fuser.tsdf_fuser_pred.tsdf
    vol.save(str(tmp_path / "scan"), "scan.bin")
    assert not vol.tsdf_values.is_cuda                       # the reference leaves the volume on the host
    a, b = (tmp_path / "m.ply").read_bytes(), (tmp_path / "scan" / "scan.ply").read_bytes()
    assert a == b and len(a) > 100
    vol.save(str(tmp_path / "again"), "scan.bin")            # meshed from a device copy
    assert (tmp_path / "again" / "scan.ply").read_bytes() == a
    assert ref.faces.shape[0] > 0


def test_refusals():
    vol = TSDF.from_bounds(dict(xmin=0, xmax=0.8, ymin=0, ymax=0.8, zmin=0, zmax=0.8), 0.1, device=DEV)
    vol.cpu()
    with pytest.raises(_lib.HipLibraryError):
        vol.extract_mesh()
    with pytest.raises(ValueError):
        marching_cubes(torch.zeros((1, 8, 8), dtype=torch.float16, device=DEV))
    with pytest.raises(ValueError):
        marching_cubes(torch.zeros((8, 8, 1), dtype=torch.float16, device=DEV))
    flat = TSDF.from_bounds(dict(xmin=0, xmax=0.8, ymin=0, ymax=0.8, zmin=0, zmax=0.8), 0.1, device=DEV).extract_mesh()
    assert flat.vertices.shape == (0, 3) and flat.faces.shape == (0, 3)
