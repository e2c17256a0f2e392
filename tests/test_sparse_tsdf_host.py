"""Host checks of the sparse TSDF (no GPU): the numpy oracle (tests/sparse_tsdf_oracle.py) against a per-voxel Python
loop of the header's rules on tiny scenes, its extraction against tests/mesh_oracle.py on a fully observed volume,
block-key packing and order, and the PLY writer / reader with vertex colours."""
import math

import numpy as np
import pytest
import torch

import mesh_oracle
import sparse_tsdf_oracle as so
from simplerecon_amd import scalable_tsdf as st
from simplerecon_amd.ply import read_ply
from simplerecon_amd.tsdf import TriangleMesh

f32 = np.float32


def _tiny_scene(seed, h=9, w=13):
    """A tilted plane with a bump in front of a camera with a small random pose; a few holes and far pixels."""
    rng = np.random.default_rng(seed)
    vv, uu = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    depth = (1.2 + 0.05 * uu - 0.03 * vv + 0.2 * np.exp(-((uu - w / 2) ** 2 + (vv - h / 2) ** 2) / 8)).astype(np.float32)
    depth[rng.random((h, w)) < 0.1] = 0
    depth[0, 4] = 7.0     # beyond max_depth
    depth[4, 0] = np.nan
    K = np.eye(4, dtype=np.float32)
    K[0, 0], K[1, 1], K[0, 2], K[1, 2] = 11.0, 10.5, w / 2 - 0.3, h / 2 + 0.2
    a, b = rng.uniform(-0.2, 0.2, 2)
    R = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]]) @ \
        np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = rng.uniform(-0.3, 0.3, 3)
    color = rng.integers(0, 256, (3, h, w), dtype=np.uint8)
    return depth, K, T.astype(np.float32), color


def _loop_touch(depth, K, T, trunc, unit):
    """Per-pixel Python floats (fp64)."""
    Kd = K.astype(np.float64)
    M = np.linalg.inv(T.astype(np.float64))
    keys = set()
    h, w = depth.shape
    for v in range(0, h, 4):
        for u in range(0, w, 4):
            d = float(depth[v, u])
            if not d > 0:
                continue
            x, y, z = ((u - Kd[0, 2]) * d) / Kd[0, 0], ((v - Kd[1, 2]) * d) / Kd[1, 1], d
            rng = []
            for a in range(3):
                p = ((M[a, 0] * x + M[a, 1] * y) + M[a, 2] * z) + M[a, 3]
                rng.append(range(math.floor((p - trunc) / unit), math.floor((p + trunc) / unit) + 1))
            for bx in rng[0]:
                for by in rng[1]:
                    for bz in rng[2]:
                        keys.add(int(so.pack([[bx, by, bz]])[0]))
    return keys


def _loop_integrate(blocks, keys, depth, K, T, color, vl, trunc):
    """Per-voxel numpy fp32 scalars, in the header's order."""
    h, w = depth.shape
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    vl, tr = f32(vl), f32(trunc)
    for key in sorted(keys):
        data = blocks.setdefault(key, np.zeros((5, so.VOXELS), np.float32))
        b = so.unpack([key])[0]
        for l in range(so.VOXELS):
            g = b * 16 + np.array([l // 256, (l // 16) % 16, l % 16])
            x, y, z = ((f32(g[0]) + f32(0.5)) * vl, (f32(g[1]) + f32(0.5)) * vl, (f32(g[2]) + f32(0.5)) * vl)
            px = ((T[0, 0] * x + T[0, 1] * y) + T[0, 2] * z) + T[0, 3]
            py = ((T[1, 0] * x + T[1, 1] * y) + T[1, 2] * z) + T[1, 3]
            pz = ((T[2, 0] * x + T[2, 1] * y) + T[2, 2] * z) + T[2, 3]
            if pz <= 0:
                continue
            uf = ((px * fx) / pz + cx) + f32(0.5)
            vf = ((py * fy) / pz + cy) + f32(0.5)
            if not (f32(0.0001) <= uf < f32(w) - f32(0.0001) and f32(0.0001) <= vf < f32(h) - f32(0.0001)):
                continue
            u, v = int(uf), int(vf)
            D = depth[v, u]
            if D <= 0:
                continue
            a = (f32(u) - cx) / fx
            bb = (f32(v) - cy) / fy
            with np.errstate(invalid="ignore"):
                sdf = (D - pz) * np.sqrt((f32(1) + a * a) + bb * bb)
            if not sdf > -tr:
                continue
            tn = min(f32(1), sdf / tr)
            W = data[1, l]
            W1 = W + f32(1)
            data[0, l] = (data[0, l] * W + tn) / W1
            for ch in range(3):
                c = f32(178) if color is None else f32(color[ch, v, u])
                data[2 + ch, l] = (data[2 + ch, l] * W + c) / W1
            data[1, l] = W1


@pytest.mark.parametrize("use_color", [False, True])
def test_oracle_matches_per_voxel_loop(use_color):
    vl, trunc, max_depth = 0.25, 0.75, 3.0
    vol = so.Volume(vl, trunc, max_depth)
    ref = {}
    for seed in (1, 2):
        depth, K, T, color = _tiny_scene(seed)
        color = color if use_color else None
        vol.integrate_frame(depth, K, T, color)
        d = so.preprocess_depth(depth, max_depth)
        keys = _loop_touch(d, K, T, trunc, 16 * vl)
        assert set(so.touch(d, K, T, trunc, 16 * vl).tolist()) == keys
        _loop_integrate(ref, keys, d, K, T, color, vl, trunc)
    k, tsdf, wgt, rgb = vol.arrays()
    assert k.tolist() == sorted(ref)
    want = np.stack([ref[x] for x in k])
    assert (wgt > 0).any()
    np.testing.assert_array_equal(tsdf, want[:, 0])
    np.testing.assert_array_equal(wgt, want[:, 1])
    np.testing.assert_array_equal(rgb, want[:, 2:5])


def test_extraction_matches_dense_oracle_on_observed_volume():
    """Eight blocks, every voxel observed, fp16-representable values: the same surface as the dense rules (which
    round through fp16), vertex for vertex and face for face up to numbering."""
    n = 32
    g = np.stack(np.meshgrid(np.arange(n), np.arange(n), np.arange(n), indexing="ij"), -1).astype(np.float64)
    vals = (np.linalg.norm(g - np.array([15.3, 16.7, 14.1]), axis=-1) - 9.6) / 3.0
    vals += 0.3 * np.sin(g[..., 0] * 0.7) * np.cos(g[..., 2] * 0.5)
    vals = np.clip(vals, -1, 1).astype(np.float16).astype(np.float32)
    coords = np.array([[i, j, k] for i in range(2) for j in range(2) for k in range(2)])
    keys = so.pack(coords)
    order = np.argsort(keys)
    keys, coords = keys[order], coords[order]
    tsdf = np.stack([vals[c[0] * 16:c[0] * 16 + 16, c[1] * 16:c[1] * 16 + 16, c[2] * 16:c[2] * 16 + 16].reshape(-1)
                     for c in coords])
    wgt = np.ones_like(tsdf)
    rgb = np.zeros((len(keys), 3, so.VOXELS), np.float32)
    verts, faces, _, vpos, vown = so.extract_mesh(keys, tsdf, wgt, rgb, 1.0)
    mverts, mfaces, _, mvpos = mesh_oracle.marching_cubes(vals, normals=False)
    assert len(verts) == len(mverts) > 1000 and len(faces) == len(mfaces) > 1000
    # our vertex -> the dense oracle's (dense numbering: linear voxel index, then axis)
    dk = ((vown[:, 0] * n + vown[:, 1]) * n + vown[:, 2]) * 3 + vown[:, 3]
    to_dense = np.argsort(np.argsort(dk))
    np.testing.assert_array_equal(vpos, mvpos[to_dense])
    np.testing.assert_array_equal(verts, (mverts[to_dense] + f32(0.5)).astype(np.float32))
    np.testing.assert_array_equal(mesh_oracle.canonical_faces(to_dense[faces]), mesh_oracle.canonical_faces(mfaces))
    # blocks in key order: the vertices of block 0 come first
    blk = np.floor_divide(vown[:, :3], 16)
    bkey = so.pack(blk)
    assert (np.diff(np.searchsorted(keys, bkey)) >= 0).all()


def test_unobserved_voxels_split_the_surface():
    """A weight-0 voxel is NaN: no vertex on its edges, no face on its cubes."""
    coords = np.array([[0, 0, 0]])
    keys = so.pack(coords)
    l = np.arange(so.VOXELS)
    z = l % 16
    tsdf = ((z - 7.5) / 4).astype(np.float32)[None]
    wgt = np.ones_like(tsdf)
    _, faces_full, _, _, _ = so.extract_mesh(keys, tsdf, wgt, np.zeros((1, 3, so.VOXELS), np.float32), 0.1)
    wgt2 = wgt.copy()
    wgt2[0, (l // 256 == 5) & ((l // 16) % 16 == 5) & (z == 7)] = 0
    v2, faces_hole, _, _, own = so.extract_mesh(keys, tsdf, wgt2, np.zeros((1, 3, so.VOXELS), np.float32), 0.1)
    assert len(faces_hole) < len(faces_full)
    assert not ((own[:, 0] == 5) & (own[:, 1] == 5) & (own[:, 2] == 7)).any()


def test_key_packing_and_order():
    rng = np.random.default_rng(3)
    coords = np.concatenate([rng.integers(-(1 << 20), 1 << 20, (500, 3)),
                             [[-(1 << 20)] * 3, [(1 << 20) - 1] * 3, [0, 0, 0], [-1, -1, -1], [0, 0, -1]]])
    keys = st.pack_keys(coords)
    np.testing.assert_array_equal(keys, so.pack(coords))
    np.testing.assert_array_equal(st.unpack_keys(keys), coords)
    lex = np.lexsort(coords.T[::-1])           # x-major lexicographic order
    np.testing.assert_array_equal(np.argsort(keys, kind="stable"), lex)
    assert (keys >= 0).all() and st.KEY_NONE < 0
    with pytest.raises(ValueError):
        st.pack_keys([[1 << 20, 0, 0]])
    with pytest.raises(ValueError):
        st.pack_keys([[0, -(1 << 20) - 1, 0]])


def _mesh(colors):
    v = torch.tensor([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1.5]], dtype=torch.float32)
    f = torch.tensor([[0, 1, 2], [0, 2, 3]], dtype=torch.int32)
    return TriangleMesh(v, f, None, colors)


def test_ply_round_trip_with_colors(tmp_path):
    c = torch.tensor([[0.0, 0.5, 1.0], [0.2, 0.3999, 0.0019], [1.2, -0.1, 0.998], [0.7, 0.7, 0.7]])
    path = str(tmp_path / "c.ply")
    _mesh(c).write_ply(path)
    head = open(path, "rb").read().split(b"end_header")[0].decode()
    assert "property uchar red\nproperty uchar green\nproperty uchar blue\nelement face 2" in head
    back = read_ply(path)
    assert isinstance(back, TriangleMesh) and back.colors is not None
    want8 = np.clip(np.floor(c.numpy() * f32(255) + f32(0.5)), 0, 255)
    np.testing.assert_array_equal(back.colors.numpy() * 255, want8.astype(np.float32) / f32(255) * f32(255))
    np.testing.assert_array_equal(np.round(back.colors.numpy() * 255), want8)
    np.testing.assert_array_equal(back.vertices.numpy(), _mesh(c).vertices.numpy())
    np.testing.assert_array_equal(back.faces.numpy(), _mesh(c).faces.numpy())


def test_ply_without_colors_keeps_the_layout(tmp_path):
    path = str(tmp_path / "p.ply")
    m = _mesh(None)
    m.write_ply(path)
    v, f = m.vertices.numpy(), m.faces.numpy()
    want = ("ply\nformat binary_little_endian 1.0\nelement vertex 4\nproperty float x\nproperty float y\n"
            "property float z\nelement face 2\nproperty list uchar int vertex_indices\nend_header\n").encode()
    want += v.astype("<f4").tobytes()
    for row in f:
        want += bytes([3]) + row.astype("<i4").tobytes()
    assert open(path, "rb").read() == want
    assert read_ply(path).colors is None


def test_reverse_imagenet_normalize_matches_mean_std():
    x = torch.rand(2, 3, 4, 5) * 4 - 2
    got = st.reverse_imagenet_normalize(x)
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    torch.testing.assert_close(got, x * std + mean, atol=1e-5, rtol=1e-5)


def test_volume_refuses_cpu():
    from simplerecon_amd._lib import HipLibraryError
    with pytest.raises(HipLibraryError):
        st.ScalableTSDFVolume(0.04, 0.12, 3.0, device="cpu")
