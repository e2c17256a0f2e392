"""GPU point-cloud fusion (csrc/sr_pcfusion.hip via simplerecon_amd.point_cloud): the reference's goldens and the fp64
oracle under the comparison rule of tests/pc_oracle.py, edge cases of the rules, chunking and run-to-run determinism,
voxel downsampling, the fuser end to end and refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import pc_cases
import pc_oracle as po
from simplerecon_amd import _lib, synthetic
from simplerecon_amd import point_cloud as pcf
from test_pc_host import read_ply

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _raw(depths, P, K, zt, ref_begin=0, ref_count=None):
    """sr_pc_consistency on one chunk: averaged points [c,h,w,3] and counts [c,h,w], as numpy."""
    N, h, w = depths.shape
    c = N - ref_begin if ref_count is None else ref_count
    D = depths.to(DEV).float().contiguous()
    consts = pcf.frame_constants(P, K).to(DEV)
    pts = torch.empty((c, h, w, 3), dtype=torch.float32, device=DEV)
    cnt = torch.empty((c, h, w), dtype=torch.int32, device=DEV)
    rc = _lib.lib().sr_pc_consistency(_lib.ptr(D), _lib.ptr(consts), N, h, w, ref_begin, c, C.c_float(zt),
                                      _lib.ptr(pts), _lib.ptr(cnt), _lib.stream_ptr(torch.device(DEV)))
    _lib.check(rc, "sr_pc_consistency")
    torch.cuda.synchronize()
    return pts.cpu().numpy(), cnt.cpu().numpy()


def _check_oracle(sc, zt, nt, max_amb=0.005, **kw):
    d, P, K, img = sc["depths"], sc["cam_T_world"], sc["K"], sc["images"]
    orc = po.fuse_scene(d.numpy(), P.numpy(), K.numpy(), zt, **kw)
    pts, rgb, valid = pcf.process_scene(d, img, P, K, zt, nt)
    _, cnt = _raw(d, P, K, zt)
    return po.compare(orc, nt, valid, pts, rgb, img.numpy(), got_n=cnt, max_amb=max_amb), valid


@pytest.mark.parametrize("name", sorted(pc_cases.CASES))
def test_goldens(name):
    sc, zt, nt = pc_cases.scene(name)
    g = np.load(os.path.join(GOLDEN, f"pcfusion_{name}.npz"))
    orc = po.fuse_scene(sc["depths"].numpy(), sc["cam_T_world"].numpy(), sc["K"].numpy(), zt)
    pts, rgb, valid = pcf.process_scene(sc["depths"], sc["images"], sc["cam_T_world"], sc["K"], zt, nt)
    amb = orc["amb"].reshape(valid.shape)
    assert not ((valid != g["all_valid"]) & ~amb).any()
    po.compare(orc, nt, valid, pts, rgb, sc["images"].numpy())
    po.compare(orc, nt, g["all_valid"], g["fused_pts"], g["fused_rgb"], sc["images"].numpy())


def test_zero_depth_and_holes():
    sc = synthetic.raycast_scene(5, 40, 56, seed=11, noise=0.001)
    sc["depths"][1, 10] = 0.0                    # a whole row of zeros: each pixel becomes the camera centre
    sc["depths"][3, :, 7] = 0.0
    _check_oracle(sc, 0.04, 2)


def test_camera_facing_away():
    sc = synthetic.raycast_scene(5, 40, 56, seed=12)
    flip = torch.diag(torch.tensor([-1.0, 1.0, -1.0, 1.0]))
    sc["cam_T_world"][2] = flip @ sc["cam_T_world"][2]   # frame 2 looks backwards: most points have z <= 1e-4 in it
    _check_oracle(sc, 0.04, 2)


def test_projection_on_last_column():
    """Two frames with the same camera: a pixel of column w-1 projects onto x = w-1 (margin 0: ambiguous in the
    oracle, as are the other border pixels of frames 0 and 1, so the designed case allows them); everything else must agree."""
    sc = synthetic.raycast_scene(3, 32, 48, seed=13)
    sc["cam_T_world"][1] = sc["cam_T_world"][0]
    sc["depths"][1] = sc["depths"][0]
    frac, valid = _check_oracle(sc, 0.04, 1, max_amb=0.12)
    assert valid[0, 1:-1, 1:-1].all()


@pytest.mark.parametrize("N", [1, 2])
def test_too_few_frames_keep_nothing(N):
    sc = synthetic.raycast_scene(N, 24, 32, seed=14)
    pts, rgb, valid = pcf.process_scene(sc["depths"], sc["images"], sc["cam_T_world"], sc["K"], 0.04, 3)
    assert pts.shape == (0, 3) and rgb.shape == (0, 3) and valid.shape == (N, 24, 32) and not valid.any()
    _check_oracle(sc, 0.04, 3)


def test_threshold_zero_keeps_everything():
    sc = synthetic.raycast_scene(4, 24, 32, seed=15, holes=0.01)
    _, valid = _check_oracle(sc, 0.04, 0)
    assert valid.all()


def test_process_depth_matches_scene_row():
    sc, zt, nt = pc_cases.scene("small")
    d, img, P, K = sc["depths"], sc["images"], sc["cam_T_world"], sc["K"]
    pts, rgb, valid = pcf.process_scene(d, img, P, K, zt, nt)
    r = 2
    src = [i for i in range(d.shape[0]) if i != r]
    p1, c1, v1 = pcf.process_depth(d[r], img[r], d[src], img[src], P[r], P[src], K[r], K[src], zt, nt)
    assert np.array_equal(v1, valid[r])
    start = int(valid[:r].sum())
    assert np.array_equal(p1, pts[start:start + len(p1)]) and np.array_equal(c1, rgb[start:start + len(p1)])


def test_chunks_and_runs_are_bitwise_equal():
    sc, zt, nt = pc_cases.scene("holes")
    args = (sc["depths"].to(DEV), sc["images"].to(DEV), sc["cam_T_world"], sc["K"], zt, nt)
    base = pcf._fuse(*args)
    again = pcf._fuse(*args)
    for a, b in zip(base, again):
        assert torch.equal(a, b)
    for chunk in (1, 3, 5):
        got = pcf._fuse(*args, chunk_frames=chunk)
        for a, b in zip(base, got):
            assert torch.equal(a, b), f"chunk {chunk}"
    p_all, n_all = _raw(sc["depths"], sc["cam_T_world"], sc["K"], zt)
    p_mid, n_mid = _raw(sc["depths"], sc["cam_T_world"], sc["K"], zt, ref_begin=3, ref_count=2)
    assert np.array_equal(p_all[3:5], p_mid) and np.array_equal(n_all[3:5], n_mid)


def test_full_size_sample_against_oracle():
    """480 x 640, N = 64: properties of the whole result, and a 1 % pixel sample against the oracle.  At 640 px one fp32
    ulp of a coordinate is 6e-5 px, so bounds margins below 1e-4 px count as ambiguous here.  No holes: with 63
    sources, a zero texel beside a .5 boundary makes about 0.7 % of the pixels ambiguous at 1 % holes (zero depths are
    covered by the smaller cases)."""
    N, h, w = 64, 480, 640
    sc = {k: v.cpu() for k, v in synthetic.raycast_scene(N, h, w, seed=16, noise=0.002, device=DEV).items()}
    zt, nt = 0.04, 3
    pts, cnt = _raw(sc["depths"], sc["cam_T_world"], sc["K"], zt)
    assert np.isfinite(pts).all()
    assert (cnt >= 0).all() and (cnt <= N - 1).all()
    kept = (cnt >= nt).mean()
    assert 0.3 < kept < 1.0, kept
    pc, valid = pcf.fuse_scene(sc["depths"], sc["images"], sc["cam_T_world"], sc["K"], zt, nt)
    assert np.array_equal(valid.cpu().numpy(), cnt >= nt) and len(pc) == int((cnt >= nt).sum())
    rng = np.random.default_rng(0)
    amb_total, sample_total = 0, 0
    for r in range(N):
        pix = rng.choice(h * w, size=h * w // 100, replace=False)
        o = po.fuse_frame(sc["depths"].numpy(), sc["cam_T_world"].numpy(), sc["K"].numpy(), r, zt, pixels=pix,
                          eps_m=1e-4)
        ok = ~o["amb"]
        amb_total += int(o["amb"].sum())
        sample_total += len(pix)
        assert np.array_equal(cnt[r].reshape(-1)[pix][ok], o["n"][ok]), f"frame {r}"
        err = np.abs(pts[r].reshape(-1, 3)[pix][ok] - o["avg"][ok]).max(1)
        assert (err <= 2e-5 + o["tol"][ok]).all(), f"frame {r}: {err.max()}"
    assert amb_total < 0.005 * sample_total


def test_voxel_down_sample_matches_oracle():
    sc, zt, nt = pc_cases.scene("holes")
    pc, _ = pcf.fuse_scene(sc["depths"], sc["images"], sc["cam_T_world"], sc["K"], zt, nt)
    for vs in (0.02, 0.05, 0.3):
        a = pc.voxel_down_sample(vs)
        b = pc.voxel_down_sample(vs)
        assert torch.equal(a.points, b.points) and torch.equal(a.colors, b.colors)
        wp, wc, _ = po.voxel_down_sample(pc.points.cpu().numpy(), pc.colors.cpu().numpy(), vs)
        gp, gc = a.points.cpu().numpy(), a.colors.cpu().numpy()
        assert gp.shape == wp.shape
        ulp = np.spacing(np.abs(wp).astype(np.float32))
        assert (np.abs(gp - wp) <= ulp).all()
        assert np.array_equal(gc, wc)
    none = pcf.PointCloud(pc.points).voxel_down_sample(0.05)
    assert none.colors is None and torch.equal(none.points, pc.voxel_down_sample(0.05).points)
    empty = pcf.PointCloud(torch.zeros((0, 3), device=DEV)).voxel_down_sample(0.05)
    assert len(empty) == 0
    with pytest.raises(ValueError):
        pc.voxel_down_sample(1e-9)                   # 2^21 voxels or more per axis


def test_fuser_end_to_end(tmp_path):
    sc = synthetic.raycast_scene(8, 48, 64, seed=17, noise=0.001)
    depth = sc["depths"][:, None].to(DEV) * 1.0
    depth[:, :, :4] = 9.0                            # beyond max_fusion_depth: zeroed by the fuser
    K44 = torch.eye(4).repeat(8, 1, 1)
    K44[:, :3, :3] = sc["K"] / 2.0
    K44[:, 2, 2] = 1.0
    half = torch.nn.functional.interpolate(depth, size=(24, 32), mode="nearest")
    g = torch.Generator().manual_seed(3)
    color = torch.randn((8, 3, 24, 32), generator=g).to(DEV)
    fuser = pcf.PointCloudFuser(z_thresh=0.04, n_consistent_thresh=2, voxel_downsample=0.05, max_fusion_depth=3.0,
                                fusion_size=(48, 64))
    for b in (0, 4):
        fuser.fuse_frames(half[b:b + 4], K44[b:b + 4].to(DEV), sc["cam_T_world"][b:b + 4].to(DEV), color[b:b + 4])
    got = fuser.get_point_cloud()
    # by hand: the same steps as pc_fusion.py:122-150
    d = half.clone()
    d[d > 3.0] = 0
    d = torch.nn.functional.interpolate(d, size=(48, 64), mode="nearest")[:, 0]
    assert (d[:, :4] == 0).all()
    K = K44.clone()
    K[:, 0] *= 2.0
    K[:, 1] *= 2.0
    img = torch.nn.functional.interpolate(color, size=(48, 64), mode="bilinear")
    img = img * torch.tensor([0.229, 0.224, 0.225], device=DEV).view(1, 3, 1, 1) + \
        torch.tensor([0.485, 0.456, 0.406], device=DEV).view(1, 3, 1, 1)
    img = (img.permute(0, 2, 3, 1) * 255).clamp(0, 255).to(torch.uint8)
    pc, _ = pcf.fuse_scene(d, img, sc["cam_T_world"], K[:, :3, :3], 0.04, 2)
    want = pc.voxel_down_sample(0.05)
    assert len(want) > 100
    assert torch.equal(got.points, want.points) and torch.equal(got.colors, want.colors)
    path = str(tmp_path / "cloud.ply")
    fuser.export_point_cloud(path)
    props, v = read_ply(path)
    assert props == ["x", "y", "z", "red", "green", "blue"]
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), want.points.cpu().numpy())
    assert np.array_equal(np.stack([v["red"], v["green"], v["blue"]], 1), want.colors.cpu().numpy())


def test_refusals(tmp_path):
    sc = synthetic.raycast_scene(3, 24, 32, seed=18)
    d, img, P, K = (sc[k].to(DEV) for k in ("depths", "images", "cam_T_world", "K"))
    with pytest.raises(ValueError):
        pcf.fuse_scene(d[:, :1], img[:, :1], P, K)                    # h < 2
    with pytest.raises(ValueError):
        pcf.fuse_scene(d[:, :, :1], img[:, :, :1], P, K)              # w < 2
    with pytest.raises(ValueError):
        pcf.fuse_scene(d, img[:2], P, K)
    with pytest.raises(ValueError):
        pcf.fuse_scene(d, img, P[:, :3], K)
    with pytest.raises(TypeError):
        pcf.fuse_scene(d, img.float(), P, K)
    fuser = pcf.PointCloudFuser()
    with pytest.raises(ValueError):
        fuser.fuse_frames(d, torch.eye(4, device=DEV)[None].repeat(3, 1, 1), P)   # depths not [B,1,h,w]
    with pytest.raises(ValueError):
        fuser.export_point_cloud(str(tmp_path / "x.obj"))
