"""Host side of the mesh metrics (no GPU): the PLY reader against both writers and hand-written files, its refusals,
the numpy oracle on hand-computed cases, the grid plan of the C library, TSDF.from_mesh bounds and the refusal of host
tensors."""
import numpy as np
import pytest
import torch

import mesh_metrics_oracle as mo
from simplerecon_amd import _lib, mesh_metrics, synthetic
from simplerecon_amd.ply import read_ply
from simplerecon_amd.point_cloud import PointCloud
from simplerecon_amd.tsdf import TSDF, TriangleMesh


def _mesh(n=50, seed=0):
    g = np.random.default_rng(seed)
    v = torch.from_numpy(g.standard_normal((n, 3)).astype(np.float32))
    f = torch.from_numpy(g.integers(0, n, (2 * n, 3)).astype(np.int32))
    return TriangleMesh(v, f)


def test_ply_round_trip_triangle_mesh(tmp_path):
    m = _mesh()
    m.normals = torch.nn.functional.normalize(torch.randn(50, 3), dim=1)
    m.write_ply(tmp_path / "m.ply")
    r = read_ply(str(tmp_path / "m.ply"))
    assert isinstance(r, TriangleMesh) and r.normals is None
    assert r.vertices.dtype == torch.float32 and r.faces.dtype == torch.int32
    assert torch.equal(r.vertices, m.vertices) and torch.equal(r.faces, m.faces)


@pytest.mark.parametrize("colors", [True, False])
def test_ply_round_trip_point_cloud(tmp_path, colors):
    pts = torch.randn(77, 3)
    cols = torch.randint(0, 256, (77, 3), dtype=torch.uint8) if colors else None
    PointCloud(pts, cols).write_ply(tmp_path / "p.ply")
    r = read_ply(tmp_path / "p.ply")
    assert isinstance(r, PointCloud) and torch.equal(r.points, pts)
    assert (r.colors is None) == (not colors)
    if colors:
        assert torch.equal(r.colors, cols)


def test_ply_round_trip_empty_mesh(tmp_path):
    TriangleMesh(torch.zeros(0, 3), torch.zeros(0, 3, dtype=torch.int32)).write_ply(tmp_path / "e.ply")
    r = read_ply(tmp_path / "e.ply")
    assert isinstance(r, TriangleMesh) and r.vertices.shape == (0, 3) and r.faces.shape == (0, 3)


ASCII = """ply
format ascii 1.0
comment hand written
element vertex 5
property double x
property double y
property double z
property uchar red
property uchar green
property uchar blue
element face 2
property list uchar int vertex_indices
end_header
0 0 0 255 0 0
1 0 0 0 255 0
1 1 0 0 0 255
0 1 0 1 2 3
0.5 0.5 1 4 5 6
3 0 1 2
4 0 2 3 4
"""


def test_ply_ascii_with_polygon_fan(tmp_path):
    (tmp_path / "a.ply").write_text(ASCII)
    r = read_ply(tmp_path / "a.ply")
    assert isinstance(r, TriangleMesh)
    np.testing.assert_array_equal(r.faces.numpy(), [[0, 1, 2], [0, 2, 3], [0, 3, 4]])
    np.testing.assert_array_equal(r.vertices.numpy()[4], np.float32([0.5, 0.5, 1]))
    (tmp_path / "b.ply").write_text(ASCII.replace("element face 2", "element face 0").rsplit("3 0 1 2", 1)[0])
    pc = read_ply(tmp_path / "b.ply")
    assert isinstance(pc, TriangleMesh) and pc.faces.shape == (0, 3)


def test_ply_scannet_style_binary(tmp_path):
    """vh_clean_2.ply layout: float xyz, uchar rgba, `list uchar int vertex_indices`."""
    g = np.random.default_rng(1)
    v = np.empty(9, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1"),
                           ("alpha", "u1")])
    xyz = g.standard_normal((9, 3)).astype(np.float32)
    for i, a in enumerate("xyz"):
        v[a] = xyz[:, i]
    for c in ("red", "green", "blue", "alpha"):
        v[c] = g.integers(0, 256, 9)
    f = np.empty(4, dtype=[("n", "u1"), ("i", "<i4", (3,))])
    f["n"] = 3
    f["i"] = g.integers(0, 9, (4, 3))
    hdr = ("ply\nformat binary_little_endian 1.0\nelement vertex 9\nproperty float x\nproperty float y\n"
           "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty uchar alpha\n"
           "element face 4\nproperty list uchar int vertex_indices\nend_header\n")
    (tmp_path / "s.ply").write_bytes(hdr.encode() + v.tobytes() + f.tobytes())
    r = read_ply(tmp_path / "s.ply")
    np.testing.assert_array_equal(r.vertices.numpy(), xyz)
    np.testing.assert_array_equal(r.faces.numpy(), f["i"])
    # the same vertices as a point cloud (no face element): colours kept, alpha skipped
    (tmp_path / "c.ply").write_bytes(hdr.split("element face")[0].encode() + b"end_header\n" + v.tobytes())
    pc = read_ply(tmp_path / "c.ply")
    np.testing.assert_array_equal(pc.colors.numpy(), np.stack([v["red"], v["green"], v["blue"]], 1))


@pytest.mark.parametrize("bad, match", [
    ("format binary_big_endian 1.0", "format"),
    ("property float32x x", "property"),
    ("elemnt vertex 5", "elemnt"),
    ("element vertex five", "element"),
])
def test_ply_refuses_bad_headers(tmp_path, bad, match):
    lines = ASCII.splitlines()
    key = bad.split()[0][:4]
    i = next(k for k, ln in enumerate(lines) if ln.startswith(key) or (key == "elem" and ln.startswith("element")))
    lines[i] = bad
    (tmp_path / "x.ply").write_text("\n".join(lines) + "\n")
    with pytest.raises(ValueError, match=match):
        read_ply(tmp_path / "x.ply")


def test_ply_refuses_bad_indices_and_short_files(tmp_path):
    (tmp_path / "i.ply").write_text(ASCII.replace("3 0 1 2", "3 0 1 5"))
    with pytest.raises(ValueError, match="outside"):
        read_ply(tmp_path / "i.ply")
    (tmp_path / "n.ply").write_text(ASCII.replace("3 0 1 2", "3 0 -1 2"))
    with pytest.raises(ValueError, match="outside"):
        read_ply(tmp_path / "n.ply")
    m = _mesh()
    m.write_ply(tmp_path / "t.ply")
    data = (tmp_path / "t.ply").read_bytes()
    (tmp_path / "t.ply").write_bytes(data[:-5])
    with pytest.raises(ValueError, match="ends"):
        read_ply(tmp_path / "t.ply")
    (tmp_path / "z.ply").write_text("plx\n")
    with pytest.raises(ValueError, match="not a PLY"):
        read_ply(tmp_path / "z.ply")


def test_oracle_hand_cases():
    # nearest neighbour with duplicates: the smallest index wins
    p = np.float32([[0, 0, 0], [1, 0, 0], [1, 0, 0], [0, 0, 0]])
    d2, i = mo.nn_fp32(np.float32([[0.9, 0, 0], [0.1, 0, 0], [0.5, 0, 0]]), p)
    np.testing.assert_array_equal(i, [1, 0, 0])
    dx = np.float32([np.float32(0.9) - np.float32(1), 0.1, 0.5])
    np.testing.assert_array_equal(d2, dx * dx)
    # threshold strictness: a distance equal to the threshold is not counted
    m = mo.metrics(np.float32([0.05, 0.01]), np.float32([0.05, 0.2, 0.0]), 0.05)
    assert m["precision"] == 0.5 and m["recall"] == 1 / 3
    assert m["f_score"] == pytest.approx(2 * 0.5 / 3 / (0.5 + 1 / 3))
    assert m["chamfer"] == pytest.approx((0.03 + 0.25 / 3) / 2)
    # an empty prediction
    e = mo.metrics(np.zeros(0, np.float32), None, 0.05)
    assert np.isnan(e["acc"]) and np.isnan(e["precision"]) and e["comp"] == np.inf and e["chamfer"] == np.inf
    assert e["recall"] == 0 and e["f_score"] == 0
    # P + R = 0
    z = mo.metrics(np.float32([1.0]), np.float32([1.0]), 0.05)
    assert z["f_score"] == 0


def test_oracle_sampler_on_its_triangles():
    m = synthetic.raycast_scene_mesh(0, spacing=0.25)
    v, f = m.vertices.numpy(), m.faces.numpy().astype(np.int64)
    pts, face, amb = mo.sample_surface(v, f, 5000, seed=3)
    assert amb.mean() < 0.01
    a, b, c = (v[f[face, k]].astype(np.float64) for k in range(3))
    n = np.cross(b - a, c - a)
    area2 = np.linalg.norm(n, axis=1)
    assert (area2 > 0).all()   # zero-area faces (sphere poles) are never chosen
    np.testing.assert_allclose(((pts - a) * n).sum(1) / area2, 0, atol=1e-5)


def test_grid_plan_rules():
    """sr_nn_grid_plan (host code of the library): about one target per cell, the cap grows the cell."""
    lib = _lib.lib()
    import ctypes as C

    def plan(n, box, cap=mesh_metrics.MAX_CELLS):
        b = (C.c_double * 6)(*box)
        cell, dims, ent = C.c_double(), (C.c_int * 3)(), C.c_int64()
        rc = lib.sr_nn_grid_plan(n, C.addressof(b), cap, C.addressof(cell), C.addressof(dims), C.addressof(ent))
        return rc, cell.value, list(dims), ent.value

    rc, h, g, e = plan(1000, [0, 0, 0, 1, 1, 1])
    assert rc == 0 and np.prod(g) >= 1000 and np.prod([np.floor(1 / (h / 0.8)) + 1] * 3) < 1000
    assert e == 512 * np.prod([(x + 7) // 8 for x in g]) + 1
    rc, h, g, e = plan(10 ** 6, [0, 0, 0, 100, 100, 0])     # a plane: one cell thick
    assert rc == 0 and g[2] == 1 and g[0] * g[1] >= 10 ** 6
    rc, h2, g2, e2 = plan(10 ** 6, [0, 0, 0, 100, 100, 0], cap=4096)
    assert rc == 0 and e2 - 1 <= 4096 and h2 > h
    rc, h, g, e = plan(5, [1, 1, 1, 1, 1, 1])               # coincident targets
    assert rc == 0 and g == [1, 1, 1]
    assert plan(5, [0, 0, 0, float("nan"), 1, 1])[0] == 1
    assert plan(5, [0, 0, 0, 1e19, 1, 1])[0] == 1
    assert plan(0, [0, 0, 0, 1, 1, 1])[0] == 1
    assert plan(5, [0, 0, 0, 1, 1, 1], cap=100)[0] == 1


def test_tsdf_from_mesh_bounds():
    v = torch.tensor([[0.1, -0.2, 0.3], [1.3, 0.8, 0.5], [0.4, 0.1, 2.0]])
    m = TriangleMesh(v, torch.tensor([[0, 1, 2]], dtype=torch.int32))
    vol = TSDF.from_mesh(m, 0.04, device="cpu")
    lo = v.double().min(0).values - 0.12
    hi = v.double().max(0).values + 0.12
    np.testing.assert_allclose(vol._origin_f32.numpy(), lo.float().numpy())
    dims = [int(np.ceil((hi[a] - lo[a]).item() / 0.04 / 8)) * 8 for a in range(3)]
    assert list(vol.tsdf_values.shape) == dims


def test_host_tensors_are_refused():
    q = torch.randn(10, 3)
    with pytest.raises(_lib.HipLibraryError):
        mesh_metrics.nearest_distances(q, q)
    with pytest.raises(_lib.HipLibraryError):
        mesh_metrics.sample_surface(_mesh(), 10)
