"""Host side of mesh export (no GPU): the PLY layout TriangleMesh.write_ply produces, and the reference's mesh-export
signatures on TSDF and OurFuser (tools/tsdf.py:158, tools/fusers_helper.py:72-81)."""
import inspect

import numpy as np
import torch

from simplerecon_amd.tsdf import TSDF, OurFuser, TriangleMesh


def read_ply(path):
    """Minimal reader of binary little-endian PLY with float vertex properties and a uchar/int face list."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv = nf = 0
    props, element = [], None
    for ln in lines[2:]:
        w = ln.split()
        if w[0] == "element":
            element = w[1]
            if element == "vertex":
                nv = int(w[2])
            else:
                nf = int(w[2])
        elif w[0] == "property" and element == "vertex":
            assert w[1] == "float"
            props.append(w[2])
        elif w[0] == "property":
            assert w[1:] == ["list", "uchar", "int", "vertex_indices"]
    vdt = np.dtype([(p, "<f4") for p in props])
    verts = np.frombuffer(data, dtype=vdt, count=nv, offset=end)
    fdt = np.dtype([("n", "u1"), ("i", "<i4", (3,))])
    faces = np.frombuffer(data, dtype=fdt, count=nf, offset=end + nv * vdt.itemsize)
    assert end + nv * vdt.itemsize + nf * fdt.itemsize == len(data)
    assert (faces["n"] == 3).all()
    return props, verts, faces["i"]


def _mesh(normals):
    g = torch.Generator().manual_seed(0)
    v = torch.rand((7, 3), generator=g) * 10 - 5
    f = torch.tensor([[0, 1, 2], [2, 3, 4], [4, 5, 6], [6, 0, 3]], dtype=torch.int32)
    n = torch.nn.functional.normalize(torch.randn((7, 3), generator=g), dim=1) if normals else None
    return TriangleMesh(v, f, n)


def test_ply_round_trip_with_normals(tmp_path):
    m = _mesh(True)
    m.write_ply(str(tmp_path / "a.ply"))
    props, v, f = read_ply(str(tmp_path / "a.ply"))
    assert props == ["x", "y", "z", "nx", "ny", "nz"]
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), m.vertices.numpy())
    assert np.array_equal(np.stack([v["nx"], v["ny"], v["nz"]], 1), m.normals.numpy())
    assert np.array_equal(f, m.faces.numpy())


def test_ply_round_trip_without_normals_and_empty(tmp_path):
    m = _mesh(False)
    m.write_ply(str(tmp_path / "b.ply"))
    props, v, f = read_ply(str(tmp_path / "b.ply"))
    assert props == ["x", "y", "z"]
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), m.vertices.numpy())
    assert np.array_equal(f, m.faces.numpy())
    e = TriangleMesh(torch.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.int32))
    e.write_ply(str(tmp_path / "c.ply"))
    _, v, f = read_ply(str(tmp_path / "c.ply"))
    assert len(v) == 0 and len(f) == 0
    c = m.cpu()
    assert c.normals is None and torch.equal(c.faces, m.faces)


def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]


def test_reference_mesh_export_signatures():
    E = inspect.Parameter.empty
    assert _params(TSDF.save) == [("self", E), ("savepath", E), ("filename", E), ("save_mesh", True)]
    assert _params(TSDF.to_mesh) == [("self", E), ("scale_to_world", True), ("export_single_mesh", False)]
    assert _params(OurFuser.export_mesh) == [("self", E), ("path", E), ("export_single_mesh", True)]
    assert _params(OurFuser.get_mesh) == [("self", E), ("export_single_mesh", True), ("convert_to_trimesh", True)]
    assert _params(TSDF.extract_mesh) == [("self", E), ("level", 0.0), ("scale_to_world", True),
                                          ("compute_normals", True)]


def test_host_volume_is_refused_without_touching_the_gpu():
    from simplerecon_amd import _lib
    from simplerecon_amd.tsdf import marching_cubes
    vol = TSDF(None, -torch.ones((8, 8, 8)), torch.zeros((8, 8, 8)), 0.1, torch.zeros(3))
    try:
        vol.extract_mesh()
    except _lib.HipLibraryError:
        pass
    else:
        raise AssertionError("a host volume must be refused")
    try:
        marching_cubes(torch.zeros((8, 8, 8)))
    except TypeError:
        pass
    else:
        raise AssertionError("fp32 volumes must be refused")
