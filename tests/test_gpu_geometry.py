"""The standalone geometry kernels (csrc/sr_geometry.hip) beyond the single 140-point block of
tests/test_gpu_api_surface.py: shapes that span several 256-thread blocks with a ragged tail, Project3D's |z| <= eps
branch in the forward and the adjoint, degenerate rays, and pose_distance on 200 poses with a trace above 3 and NaN poses
(also through sr_geom_kernel of csrc/sr_dot_volume.hip, which computes the same measures for the MLP's pose channels).
References are float64 ATen on the CPU (the restatements of tests/test_gpu_api_surface.py); bounds are that module's
(1e-6 back-projection and rays, 1e-5 projection and adjoints, its pose-measure tolerances)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import oracle
from parity import assert_close
from simplerecon_amd import geometry, synthetic
from simplerecon_amd.cost_volume import FeatureVolumeManager
from test_gpu_api_surface import _torch_backproject, _torch_project

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cameras(B, h, w, seed):
    inp = synthetic.cost_volume_inputs(B, 2, 4, h, w, seed=seed)
    return dict(invK=inp["cur_invK"], K=inp["src_Ks"][:, 1].contiguous(), T=inp["src_extrinsics"][:, 1].contiguous(),
                pose=inp["src_poses"][:, 1].contiguous())


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("h,w", [(19, 23), (33, 47)])
def test_multi_block_shapes(B, h, w):
    """437 points = 2 blocks, 1551 points = 7 blocks, both with a ragged last block; images 1 and 2 of a batch."""
    N = h * w
    assert N > 256 and N % 256 != 0
    cam = _cameras(B, h, w, seed=6)
    g = torch.Generator(device="cpu").manual_seed(100 * B + h)
    depth = 0.5 + 3.0 * torch.rand((B, 1, h, w), generator=g)
    cot_p = torch.randn((B, 4, N), generator=g)
    cot_c = torch.randn((B, 3, N), generator=g)
    d = {k: v.to(DEV) for k, v in cam.items()}
    r = {k: v.double() for k, v in cam.items()}
    bp, pr = geometry.BackprojectDepth(h, w).to(DEV), geometry.Project3D().to(DEV)

    # forward + both adjoints through the composition the reference's losses differentiate
    depth_d = depth.to(DEV).requires_grad_(True)
    pts = bp(depth_d, d["invK"])
    cam_d = pr(pts, d["K"], d["T"])
    (cam_d * cot_c.to(DEV)).sum().backward()
    depth_r = depth.double().requires_grad_(True)
    pts_r = _torch_backproject(depth_r, r["invK"], h, w)
    pts_r.retain_grad()
    cam_r = _torch_project(pts_r, r["K"], r["T"])
    (cam_r * cot_c.double()).sum().backward()
    assert pts_r.dtype == torch.float64 and not pts_r.is_cuda
    assert_close(pts.detach(), pts_r.detach(), tol=1e-6, what="BackprojectDepth")
    assert_close(cam_d.detach(), cam_r.detach(), tol=1e-5, what="Project3D")
    assert_close(depth_d.grad, depth_r.grad, tol=1e-5, what="d loss / d depth (both adjoints)")
    pts_leaf = pts.detach().clone().requires_grad_(True)
    (pr(pts_leaf, d["K"], d["T"]) * cot_c.to(DEV)).sum().backward()
    assert_close(pts_leaf.grad, pts_r.grad, tol=1e-5, what="d loss / d points")
    # the back-projection's adjoint alone, with a cotangent on all four rows (the homogeneous row carries no gradient)
    depth_d2 = depth.to(DEV).requires_grad_(True)
    (bp(depth_d2, d["invK"]) * cot_p.to(DEV)).sum().backward()
    depth_r2 = depth.double().requires_grad_(True)
    (_torch_backproject(depth_r2, r["invK"], h, w) * cot_p.double()).sum().backward()
    assert_close(depth_d2.grad, depth_r2.grad, tol=1e-5, what="d loss / d depth (back-projection alone)")

    # rays, world frame and camera frame
    wpts = pts.detach()[:, :3].contiguous()
    wpts_r = wpts.cpu().double()
    rays = geometry.get_camera_rays(d["pose"], wpts, in_camera_frame=False)
    assert_close(rays, F.normalize(wpts_r - r["pose"][:, :3, 3][:, :, None], dim=1), tol=1e-6, what="rays (world frame)")
    rays_c = geometry.get_camera_rays(None, wpts, in_camera_frame=True, cam_T_world_b44=d["T"])
    ref_c = F.normalize(torch.matmul(r["T"][:, :3, :4], torch.cat([wpts_r, torch.ones_like(wpts_r[:, :1])], 1)), dim=1)
    assert_close(rays_c, ref_c, tol=1e-6, what="rays (camera frame)")


def _project_bwd_f64(g, pts, K, T, eps):
    """Adjoint of Project3D in the points as the kernel states it (the scale of the |z| <= eps branch is a constant):
    d_q = (g_x s, g_y s, g_z - [|q_z| > eps] (g_x q_x + g_y q_y) s^2), d_X = P^T d_q, in float64."""
    P = (K @ T)[:, :3]
    q = P @ pts
    far = q[:, 2].abs() > eps
    s = torch.where(far, 1.0 / torch.where(far, q[:, 2] + eps, torch.ones_like(q[:, 2])), torch.ones_like(q[:, 2]))
    dq = torch.stack([g[:, 0] * s, g[:, 1] * s,
                      g[:, 2] - torch.where(far, (g[:, 0] * q[:, 0] + g[:, 1] * q[:, 1]) * s * s, torch.zeros_like(s))], 1)
    return P.transpose(1, 2) @ dq


@pytest.mark.parametrize("eps", [1e-8, 1e-3])
def test_project3d_small_depth_branch(eps):
    """K = [[f,0,cx,0],[0,f,cy,0],[0,0,1,0],[0,0,0,1]] and T = I make q_z the point's z exactly in fp32, so the float64
    reference takes the same branch as the kernel at z in {0, +-eps/2, +-eps, +-2 eps, -1} (eps as the fp32 number the
    module's buffer holds).  Each z is compared on its own: range-relative errors of one group say nothing about another
    whose values are 1e8 times smaller."""
    e32 = np.float32(eps)
    zs = np.array([0.0, e32 / 2, -e32 / 2, e32, -e32, 2 * e32, -2 * e32, -1.0], dtype=np.float32)
    in_band = [True, True, True, True, True, False, False, False]
    B, per = 2, 40
    N = per * len(zs)
    assert N > 256
    rng = np.random.default_rng(17)
    pts = np.ones((B, 4, N), np.float32)
    pts[:, :2] = rng.uniform(-1, 1, size=(B, 2, N)).astype(np.float32)
    pts[:, 2] = np.tile(zs, per)                      # point n has z = zs[n % 8]: every block holds every z
    Km = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    Km[:, 0, 0] = Km[:, 1, 1] = 21.5
    Km[:, 0, 2], Km[:, 1, 2] = 11.5, 9.5
    T = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    cot = rng.standard_normal((B, 3, N)).astype(np.float32)
    pts_t, K_t, T_t, cot_t = (torch.from_numpy(a) for a in (pts, Km, T, cot))
    pr = geometry.Project3D(eps=eps).to(DEV)
    x = pts_t.to(DEV).requires_grad_(True)
    out = pr(x, K_t.to(DEV), T_t.to(DEV))
    (out * cot_t.to(DEV)).sum().backward()
    ref = _torch_project(pts_t.double(), K_t.double(), T_t.double(), eps=float(e32))
    ref_g = _project_bwd_f64(cot_t.double(), pts_t.double(), K_t.double(), T_t.double(), float(e32))
    assert torch.isfinite(out).all() and torch.isfinite(x.grad).all()
    out_c, grad_c = out.detach().cpu(), x.grad.cpu()
    for i, (z, band) in enumerate(zip(zs, in_band)):
        sel = slice(i, N, len(zs))
        assert_close(out_c[:, :, sel], ref[:, :, sel], tol=1e-5, what=f"Project3D at z = {z:g}")
        assert_close(grad_c[:, :, sel], ref_g[:, :, sel], tol=1e-5, what=f"Project3D adjoint at z = {z:g}")
        if band:
            # (q_x, q_y, q_z + eps), unscaled; d_q_z = g_z: with P = K the z row of d_X is cx g_x + cy g_y + g_z
            q_xy = torch.stack([21.5 * pts_t[:, 0, sel].double() + 11.5 * float(z), 21.5 * pts_t[:, 1, sel].double() + 9.5 * float(z)], 1)
            assert torch.allclose(out_c[:, :2, sel].double(), q_xy, rtol=1e-6, atol=1e-30), f"unscaled pixels at z = {z:g}"
            assert torch.equal(out_c[:, 2, sel], torch.full_like(out_c[:, 2, sel], float(np.float32(z + e32))))
            dz = 11.5 * cot_t[:, 0, sel].double() + 9.5 * cot_t[:, 1, sel].double() + cot_t[:, 2, sel].double()
            assert torch.allclose(grad_c[:, 2, sel].double(), dz, rtol=1e-5, atol=1e-6), f"d_q_z = g_z at z = {z:g}"


def test_camera_rays_of_a_point_at_the_camera_centre_are_zero():
    B, N, at = 2, 437, 300
    rng = np.random.default_rng(23)
    pts = rng.uniform(-2, 2, size=(B, 3, N)).astype(np.float32)
    pose = np.tile(np.eye(4, dtype=np.float32), (B, 1, 1))
    pose[:, :3, 3] = rng.uniform(-1, 1, size=(B, 3)).astype(np.float32)
    pts_w = pts.copy()
    pts_w[:, :, at] = pose[:, :3, 3]                   # world frame: the point is the centre of world_T_cam
    pts_c = pts.copy()
    pts_c[:, :, at] = -pose[:, :3, 3]                  # camera frame, cam_T_world = (I | t): I X + t = 0 exactly
    pose_t = torch.from_numpy(pose)
    for frame, p in ((False, pts_w), (True, pts_c)):
        p_t = torch.from_numpy(p)
        if frame:
            rays = geometry.get_camera_rays(None, p_t.to(DEV), in_camera_frame=True, cam_T_world_b44=pose_t.to(DEV))
            ref = F.normalize(p_t.double() + pose_t.double()[:, :3, 3][:, :, None], dim=1)
        else:
            rays = geometry.get_camera_rays(pose_t.to(DEV), p_t.to(DEV), in_camera_frame=False)
            ref = F.normalize(p_t.double() - pose_t.double()[:, :3, 3][:, :, None], dim=1)
        assert torch.isfinite(rays).all()
        assert bool((rays[:, :, at] == 0).all()) and bool((ref[:, :, at] == 0).all())
        assert_close(rays, ref, tol=1e-6, what=f"rays (in_camera_frame={frame})")


def test_pose_distance_blocks_clamp_and_nan():
    """200 poses = 4 blocks of 64.  Pose 70 has a trace that rounds above 3 (R_measure = 0 after the clamp); pose 130 has a
    NaN rotation and a finite translation (R_measure and the distance are NaN, t_measure is not); pose 199 is all NaN (a
    tracking drop-out).  The device agrees with the host path of the same function and with the float64 ATen formula,
    torch.minimum propagating NaN, including WHICH outputs are NaN."""
    n = 200
    rng = np.random.default_rng(31)
    poses = np.tile(np.eye(4), (n, 1, 1))
    for i in range(n):
        poses[i, :3, :3] = synthetic._small_rot(rng, 0.02 if i % 2 else 1.0)
        poses[i, :3, 3] = rng.normal(size=3) * 0.3
    poses = poses.astype(np.float32)
    up = np.nextafter(np.float32(1), np.float32(2))
    poses[70, :3, :3] = np.diag([up, up, up])
    assert (poses[70, 0, 0] + poses[70, 1, 1]) + poses[70, 2, 2] > np.float32(3)
    poses[130, :3, :3] = np.nan
    poses[199] = np.nan
    T = torch.from_numpy(poses)
    dev = [v.cpu() for v in geometry.pose_distance(T.to(DEV))]
    host = geometry.pose_distance(T)
    assert all(not v.is_cuda for v in host)
    T64 = T.double()
    tr = T64[:, 0, 0] + T64[:, 1, 1] + T64[:, 2, 2]
    rm_r = torch.sqrt(2 * (1 - torch.minimum(tr, torch.tensor(3.0, dtype=torch.float64)) / 3))
    tm_r = T64[:, :3, 3].norm(dim=1)
    ref = (torch.sqrt(tm_r ** 2 + rm_r ** 2), rm_r, tm_r)
    nan_want = {130: (True, True, False), 199: (True, True, True)}
    for name, d, h, r in zip(("distance", "R_measure", "t_measure"), dev, host, ref):
        assert d.shape == (n,)
        assert torch.equal(torch.isnan(d), torch.isnan(r)), f"{name}: NaN pattern differs from the float64 formula"
        assert torch.equal(torch.isnan(d), torch.isnan(h)), f"{name}: NaN pattern differs from the host path"
    for i, want in nan_want.items():
        assert tuple(bool(torch.isnan(v[i])) for v in dev) == want, i
    ok = ~torch.isnan(ref[0])
    assert int(ok.sum()) == n - 2
    (dist, rm, tm), (dist_h, rm_h, tm_h) = [[v[ok] for v in dev], [v[ok] for v in host]]
    rm_r, tm_r = rm_r[ok].float(), tm_r[ok].float()
    # R_measure = sqrt(2 (1 - tr/3)) cancels catastrophically near the identity: compare squared values
    assert torch.allclose(tm, tm_r, rtol=1e-6) and torch.allclose(rm ** 2, rm_r ** 2, atol=2e-7)
    assert torch.allclose(dist ** 2, tm_r ** 2 + rm_r ** 2, rtol=1e-5, atol=2e-7)
    assert torch.allclose(tm_h, tm, rtol=1e-6) and torch.allclose(rm_h ** 2, rm ** 2, atol=2e-7)
    assert float(dev[1][70]) == 0.0 and float(host[1][70]) == 0.0 and float(ref[1][70]) == 0.0


def test_metadata_sweep_pose_channels_keep_a_nan_rotation():
    """sr_geom_kernel clamps the trace like sr_pose_distance_kernel: a source pose with a NaN rotation (finite translation,
    finite extrinsics) makes R_measure and the pose distance NaN, so every MLP input vector holds a NaN and the whole
    volume is NaN -- on the device as in the oracle (np.minimum) and in the reference (torch.minimum)."""
    B, K, C, D, h, w = 1, 2, 16, 2, 6, 8
    inp = synthetic.cost_volume_inputs(B, K, C, h, w, seed=41)
    inp["src_poses"][0, 1, :3, :3] = float("nan")
    mgr = FeatureVolumeManager(h, w, num_depth_bins=D, matching_dim_size=C, num_source_views=K)
    synthetic.seeded_fill_(mgr.mlp, seed=3)
    sd = {k: v.numpy() for k, v in mgr.mlp.state_dict().items()}
    mlp = dict(W1=sd["net.0.weight"], b1=sd["net.0.bias"], W2=sd["net.2.weight"], b2=sd["net.2.bias"],
               W3=sd["net.4.weight"], b3=sd["net.4.bias"])
    mgr = mgr.to(DEV)
    with torch.inference_mode():
        vol, _, planes, _ = mgr(**{k: v.to(DEV) for k, v in inp.items()})
    n = {k: v.numpy() for k, v in inp.items()}
    cv_o = oracle.mlp_volume(n["cur_feats"], n["src_feats"], n["src_Ks"], n["src_extrinsics"], n["src_poses"],
                             n["cur_invK"], planes[:, :, 0, 0].cpu().numpy(), mlp)[0]
    assert np.isnan(cv_o).all()
    assert bool(torch.isnan(vol).all())
