"""The PLY writer (simplerecon_amd.ply.write_ply behind TriangleMesh.write_ply and PointCloud.write_ply; no GPU): every
file byte for byte against a header string and a numpy record array written out here, then read back with read_ply."""
import numpy as np
import pytest
import torch

from simplerecon_amd.ply import read_ply
from simplerecon_amd.point_cloud import PointCloud
from simplerecon_amd.tsdf import TriangleMesh


def _expected(vertex_fields, columns, faces):
    """vertex_fields: [(PLY type, numpy dtype, name)], columns: {name: [V] array}, faces: [F,3] or None."""
    n = len(columns["x"])
    head = ["ply", "format binary_little_endian 1.0", f"element vertex {n}"]
    head += [f"property {ply_type} {name}" for ply_type, _, name in vertex_fields]
    rec = np.zeros(n, dtype=[(name, dt) for _, dt, name in vertex_fields])
    for name in rec.dtype.names:
        rec[name] = columns[name]
    body = rec.tobytes()
    if faces is not None:
        head += [f"element face {len(faces)}", "property list uchar int vertex_indices"]
        frec = np.zeros(len(faces), dtype=[("n", "u1"), ("i", "<i4", (3,))])
        frec["n"] = 3
        frec["i"] = faces
        body += frec.tobytes()
    return ("\n".join(head + ["end_header"]) + "\n").encode("ascii") + body


def _fields(names, ply_type, dt):
    return [(ply_type, dt, n) for n in names]


def _inputs(n, nf):
    g = np.random.default_rng(n)
    v = g.standard_normal((n, 3)).astype(np.float32)
    nrm = g.standard_normal((n, 3)).astype(np.float32)
    # colours in and outside [0, 1], and the rounding ties k + 0.5 of c * 255
    col = np.concatenate([g.random((n, 3)).astype(np.float32)[: max(n - 2, 0)],
                          np.array([[-0.25, 1.5, 0.5 / 255], [1.0, 0.0, 126.5 / 255]], np.float32)[: min(n, 2)]])
    f = g.integers(0, max(n, 1), (nf, 3)).astype(np.int32)
    return v, nrm, col, f


@pytest.mark.parametrize("n,nf", [(5, 2), (0, 0)])
@pytest.mark.parametrize("extras", [True, False])
def test_triangle_mesh_file_bytes(tmp_path, n, nf, extras):
    v, nrm, col, f = _inputs(n, nf)
    mesh = TriangleMesh(torch.from_numpy(v), torch.from_numpy(f), torch.from_numpy(nrm) if extras else None,
                        torch.from_numpy(col) if extras else None)
    path = tmp_path / "m.ply"
    mesh.write_ply(path)
    fields = _fields("xyz", "float", "<f4")
    columns = {a: v[:, i] for i, a in enumerate("xyz")}
    if extras:
        fields += _fields(("nx", "ny", "nz"), "float", "<f4") + _fields(("red", "green", "blue"), "uchar", "u1")
        columns.update({a: nrm[:, i] for i, a in enumerate(("nx", "ny", "nz"))})
        c8 = np.clip(np.floor(col * np.float32(255) + np.float32(0.5)), 0, 255).astype(np.uint8)
        columns.update({a: c8[:, i] for i, a in enumerate(("red", "green", "blue"))})
        if n:
            assert c8[-2].tolist() == [0, 255, 1] and c8[-1].tolist() == [255, 0, 127]
    assert path.read_bytes() == _expected(fields, columns, f)
    back = read_ply(path)
    assert isinstance(back, TriangleMesh) and back.normals is None
    assert torch.equal(back.vertices, mesh.vertices) and torch.equal(back.faces, mesh.faces)
    if extras:
        assert torch.equal(back.colors, torch.from_numpy(c8.astype(np.float32) / np.float32(255)))
    else:
        assert back.colors is None


@pytest.mark.parametrize("n", [5, 0])
@pytest.mark.parametrize("colors", [True, False])
def test_point_cloud_file_bytes(tmp_path, n, colors):
    v = _inputs(n, 0)[0]
    c8 = np.random.default_rng(7).integers(0, 256, (n, 3)).astype(np.uint8)
    pc = PointCloud(torch.from_numpy(v), torch.from_numpy(c8) if colors else None)
    path = tmp_path / "p.ply"
    pc.write_ply(path)
    fields = _fields("xyz", "float", "<f4")
    columns = {a: v[:, i] for i, a in enumerate("xyz")}
    if colors:
        fields += _fields(("red", "green", "blue"), "uchar", "u1")
        columns.update({a: c8[:, i] for i, a in enumerate(("red", "green", "blue"))})
    assert path.read_bytes() == _expected(fields, columns, None)
    back = read_ply(path)
    assert isinstance(back, PointCloud) and torch.equal(back.points, pc.points)
    assert torch.equal(back.colors, pc.colors) if colors else back.colors is None
