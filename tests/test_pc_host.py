"""Host side of point-cloud fusion (no GPU): the fp64 oracle against the reference's own outputs, the voxel rules on
hand-made points, the PLY layout, the C ABI's declarations and its argument refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import pc_cases
import pc_oracle as po
from simplerecon_amd import _lib
from simplerecon_amd.point_cloud import PointCloud, PointCloudFuser, frame_constants, fuse_scene

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def read_ply(path):
    """Minimal reader of a binary little-endian PLY vertex element with float / uchar properties."""
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    nv, props = 0, []
    for ln in lines[2:-1]:
        w = ln.split()
        if w[0] == "element":
            assert w[1] == "vertex"
            nv = int(w[2])
        else:
            assert w[0] == "property"
            props.append((w[2], {"float": "<f4", "uchar": "u1"}[w[1]]))
    dt = np.dtype(props)
    assert end + nv * dt.itemsize == len(data)
    return [p[0] for p in props], np.frombuffer(data, dtype=dt, count=nv, offset=end)


@pytest.mark.parametrize("name", sorted(pc_cases.CASES))
def test_oracle_matches_reference_goldens(name):
    sc, zt, nt = pc_cases.scene(name)
    g = np.load(os.path.join(GOLDEN, f"pcfusion_{name}.npz"))
    orc = po.fuse_scene(sc["depths"].numpy(), sc["cam_T_world"].numpy(), sc["K"].numpy(), zt)
    po.compare(orc, nt, g["all_valid"], g["fused_pts"], g["fused_rgb"], sc["images"].numpy())


def test_ply_round_trip(tmp_path):
    g = torch.Generator().manual_seed(0)
    pc = PointCloud(torch.randn((9, 3), generator=g), torch.randint(0, 256, (9, 3), generator=g, dtype=torch.uint8))
    pc.write_ply(str(tmp_path / "a.ply"))
    props, v = read_ply(str(tmp_path / "a.ply"))
    assert props == ["x", "y", "z", "red", "green", "blue"]
    assert v.dtype.itemsize == 15
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), pc.points.numpy())
    assert np.array_equal(np.stack([v["red"], v["green"], v["blue"]], 1), pc.colors.numpy())
    PointCloud(torch.zeros((0, 3))).write_ply(str(tmp_path / "b.ply"))
    props, v = read_ply(str(tmp_path / "b.ply"))
    assert props == ["x", "y", "z"] and len(v) == 0


def test_voxel_oracle_by_hand():
    v = 0.5
    # min_bound = (0, 0, 0) - 0.25: x = 0.25 lies exactly on the edge between voxels 0 and 1
    pts = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [0.2, 0.1, 0.0], [2.0, 1.0, 0.5], [0.0, 0.0, 0.3]], np.float32)
    cols = np.array([[0, 0, 0], [10, 11, 12], [1, 2, 3], [200, 100, 50], [255, 254, 1]], np.uint8)
    p, c, keys = po.voxel_down_sample(pts, cols, v)
    # voxels: (0,0,0) <- points 0, 2; (0,0,1) <- point 4; (1,0,0) <- point 1; (4,2,1) <- point 3
    assert keys.tolist() == [0, 1, 1 << 42, (4 << 42) | (2 << 21) | 1]
    assert np.array_equal(p[0], np.float32([0.1, 0.05, 0.0]))
    assert np.array_equal(p[1:], pts[[4, 1, 3]])                      # one-point voxels keep the point
    assert c[0].tolist() == [1, 1, 2]                                  # (0+1+1)//2, (0+2+1)//2, (0+3+1)//2: half up
    assert np.array_equal(c[1:], cols[[4, 1, 3]])


def test_frame_constants_layout():
    sc, _, _ = pc_cases.scene("small")
    c = frame_constants(sc["cam_T_world"], sc["K"]).double().numpy()
    assert c.shape == (6, 36)
    P, K = sc["cam_T_world"].double().numpy(), sc["K"].double().numpy()
    X = np.array([0.3, -0.2, 1.7])
    q = K[2] @ (P[2, :3, :3] @ X + P[2, :3, 3])
    assert np.allclose(c[2, :12].reshape(3, 4) @ np.append(X, 1), q, rtol=1e-6)
    Y = P[2, :3, :3].T @ (np.linalg.inv(K[2]) @ (2.0 * np.array([10.5, 20.25, 1.0])) - P[2, :3, 3])
    assert np.allclose(2.0 * c[2, 12:21].reshape(3, 3) @ [10.5, 20.25, 1.0] + c[2, 21:24], Y, rtol=1e-6)


def test_symbols_declared_and_bound():
    hdr = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "simplerecon_hip.h")).read()
    lib = _lib.lib()
    for name in ("sr_pc_consistency", "sr_pc_voxel_keys", "sr_pc_voxel_mean"):
        assert f"{name}(" in hdr and name in _lib.SIGNATURES
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert "#define SR_PC_FRAME_FLOATS 36" in hdr


def test_library_refuses_bad_arguments():
    """Every refusal happens before a launch, so these run without a GPU (the pointers are never read)."""
    lib = _lib.lib()
    p = C.c_void_p(16)
    f = C.c_float
    ok = dict(N=4, h=8, w=8, b=0, c=4, z=0.04)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.sr_pc_consistency(p, p, a["N"], a["h"], a["w"], a["b"], a["c"], f(a["z"]), p, p, None)
    assert call(N=0) == 1 and call(h=1) == 1 and call(w=1) == 1
    assert call(b=1) == 1 and call(c=0) == 1 and call(b=-1, c=1) == 1
    assert call(z=0.0) == 1 and call(z=-1.0) == 1 and call(z=float("inf")) == 1 and call(z=float("nan")) == 1
    assert call(N=1, h=20000, w=20000, c=1) == 1                       # 4.8 GB per frame: past int32 offsets
    assert lib.sr_pc_consistency(None, p, 4, 8, 8, 0, 4, f(0.04), p, p, None) == 1
    d = C.c_double
    assert lib.sr_pc_voxel_keys(p, 10, d(0), d(0), d(0), d(0.0), p, None) == 1
    assert lib.sr_pc_voxel_keys(p, 10, d(float("nan")), d(0), d(0), d(0.1), p, None) == 1
    assert lib.sr_pc_voxel_keys(None, 10, d(0), d(0), d(0), d(0.1), p, None) == 1
    assert lib.sr_pc_voxel_mean(p, None, 10, p, p, 11, p, None, None) == 1   # more voxels than points


def test_python_refusals_without_gpu(tmp_path):
    sc, _, _ = pc_cases.scene("small")
    with pytest.raises(ValueError):
        fuse_scene(sc["depths"][0], sc["images"], sc["cam_T_world"], sc["K"])
    with pytest.raises(ValueError):
        fuse_scene(sc["depths"][:, :1], sc["images"][:, :1], sc["cam_T_world"], sc["K"])
    with pytest.raises(ValueError):
        fuse_scene(sc["depths"], sc["images"], sc["cam_T_world"][:3], sc["K"])
    with pytest.raises(ValueError):
        fuse_scene(sc["depths"], sc["images"], sc["cam_T_world"], sc["K"], z_thresh=0.0)
    with pytest.raises(ValueError):
        PointCloudFuser().export_point_cloud(str(tmp_path / "a.pcd"))
    with pytest.raises(ValueError):
        PointCloud(torch.zeros((3, 3))).voxel_down_sample(0.0)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.HipLibraryError):
            fuse_scene(sc["depths"], sc["images"], sc["cam_T_world"], sc["K"])
        with pytest.raises(_lib.HipLibraryError):
            PointCloud(torch.zeros((3, 3))).voxel_down_sample(0.1)
