"""The HIP mesh metrics (csrc/sr_meshmetrics.hip via simplerecon_amd.mesh_metrics) against brute force and the numpy
oracle (tests/mesh_metrics_oracle.py): nearest-neighbour d2, distances and indices bit for bit on a set of hard point
layouts, the metric reduction, the surface sampler, determinism, the fusion pipeline scored end to end against the
analytic ground truth of synthetic.raycast_scene, and evaluate()'s mesh scores."""
import json
import os

import numpy as np
import pytest
import torch

import mesh_metrics_oracle as mo
from simplerecon_amd import mesh_metrics as mm
from simplerecon_amd import point_cloud, synthetic
from simplerecon_amd.point_cloud import PointCloud
from simplerecon_amd.tsdf import OurFuser, TriangleMesh

DEV = "cuda"


def _brute(q, p, chunk=1024):
    """fp32 brute force on the GPU, one elementwise torch op at a time (no contraction): (d2, index of the first
    minimum)."""
    d2 = torch.empty(len(q), dtype=torch.float32, device=q.device)
    idx = torch.empty(len(q), dtype=torch.int64, device=q.device)
    for s in range(0, len(q), chunk):
        qq = q[s:s + chunk]
        dx = qq[:, None, 0] - p[None, :, 0]
        dy = qq[:, None, 1] - p[None, :, 1]
        dz = qq[:, None, 2] - p[None, :, 2]
        d = torch.add(torch.add(torch.mul(dx, dx), torch.mul(dy, dy)), torch.mul(dz, dz))
        m, i = d.min(1)
        d2[s:s + chunk], idx[s:s + chunk] = m, i
    return d2, idx


def _gen(rng, n, scale=1.0):
    return torch.from_numpy((rng.random((n, 3)) * scale).astype(np.float32))


def _cases():
    rng = np.random.default_rng(11)
    cases = {}
    cases["uniform"] = (_gen(rng, 100_000, 3.0), _gen(rng, 100_000, 3.0) - 0.1)
    mesh = synthetic.raycast_scene_mesh(0, spacing=0.1)
    g = np.random.default_rng(5)
    v, f = mesh.vertices.numpy(), mesh.faces.numpy()
    sp = lambda n, s: torch.from_numpy(mo.sample_surface(v, f, n, seed=s)[0])   # noqa: E731
    cases["surface"] = (sp(50_000, 1), sp(50_000, 2))
    ball = g.standard_normal((20_000, 3))
    ball = ball / np.linalg.norm(ball, axis=1, keepdims=True) * 0.1 * g.random((20_000, 1)) ** (1 / 3)
    far = g.standard_normal((5_000, 3))
    far = far / np.linalg.norm(far, axis=1, keepdims=True) * g.uniform(5, 20, (5_000, 1))
    cases["far"] = (torch.from_numpy(far.astype(np.float32)), torch.from_numpy(ball.astype(np.float32)))
    base = _gen(rng, 1_000)
    dup = base[torch.from_numpy(g.integers(0, 1_000, 5_000))]
    cases["duplicates"] = (torch.cat([dup[:2_000], _gen(rng, 2_000)]), dup)
    cases["single"] = (_gen(rng, 3_000, 4.0) - 2, torch.tensor([[0.25, -0.5, 1.0]]))
    t = _gen(rng, 20_000)
    cases["equal"] = (t[torch.from_numpy(g.permutation(20_000))], t)
    pl = _gen(rng, 30_000, 2.0)
    pl[:, 2] = 0.375
    cases["plane"] = (_gen(rng, 10_000, 2.0) - torch.tensor([0.0, 0.0, 0.6]), pl)
    spread = _gen(rng, 3_000, 100.0)
    ii = torch.arange(20_000)
    cluster = torch.stack([(ii % 30).float(), (ii // 30 % 30).float(), (ii // 900).float()], 1) * 0.01 + 40.0
    cases["cluster"] = (torch.cat([_gen(rng, 10_000, 100.0), cluster[::3] + 0.004]), torch.cat([spread, cluster]))
    out = _gen(rng, 4_000, 1.0)
    q = []
    for a in range(3):
        for s in (-1, 1):
            x = _gen(rng, 500, 1.0)
            x[:, a] = 0.5 + s * (0.6 + 2 * x[:, a])
            q.append(x)
    cases["outside"] = (torch.cat(q), out)
    return cases


CASES = _cases()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_nearest_bit_exact(name):
    q, p = (x.to(DEV).contiguous() for x in CASES[name])
    max_cells = 4096 if name == "cluster" else mm.MAX_CELLS   # a small table: the cap has to grow the cell
    d2, dist, idx = mm._nearest(q, p, want_d2=True, want_dist=True, want_index=True, max_cells=max_cells)
    bd2, bidx = _brute(q, p)
    np.testing.assert_array_equal(d2.cpu().numpy().view(np.int32), bd2.cpu().numpy().view(np.int32))
    np.testing.assert_array_equal(idx.cpu().numpy(), bidx.cpu().numpy())
    np.testing.assert_array_equal(dist.cpu().numpy().view(np.int32),
                                  np.sqrt(bd2.cpu().numpy()).astype(np.float32).view(np.int32))
    if name in ("uniform", "far"):
        pd, pi = mm.nearest_distances(q, p, return_index=True)
        assert torch.equal(pd, dist) and torch.equal(pi, idx)


@pytest.mark.gpu
def test_nearest_refusals():
    p = torch.rand(100, 3, device=DEV)
    q = torch.rand(10, 3, device=DEV)
    with pytest.raises(ValueError):
        mm.nearest_distances(q, p[:0])
    bad = q.clone()
    bad[3, 1] = float("nan")
    with pytest.raises(ValueError):
        mm.nearest_distances(bad, p)
    with pytest.raises(ValueError):
        mm.nearest_distances(q, torch.where(p > 0.5, float("inf"), p))
    assert mm.nearest_distances(q[:0], p).shape == (0,)


@pytest.mark.gpu
def test_metrics_match_oracle():
    rng = np.random.default_rng(3)
    gt = _gen(rng, 30_000, 2.0)
    pred = gt[:20_000] + torch.from_numpy(rng.normal(0, 0.03, (20_000, 3)).astype(np.float32))
    pred = torch.cat([pred, _gen(rng, 2_000, 2.0) + 1.5])
    got = mm.mesh_metrics(PointCloud(pred.to(DEV)), PointCloud(gt.to(DEV)), threshold=0.05)
    dpg = np.sqrt(_brute(pred.to(DEV), gt.to(DEV))[0].cpu().numpy())
    dgp = np.sqrt(_brute(gt.to(DEV), pred.to(DEV))[0].cpu().numpy())
    want = mo.metrics(dpg, dgp, 0.05)
    assert got["precision"] == (dpg < np.float32(0.05)).sum() / len(pred)   # the counts, exactly
    assert got["recall"] == (dgp < np.float32(0.05)).sum() / len(gt)
    for k in mo.KEYS:
        np.testing.assert_allclose(got[k], want[k], rtol=1e-12, atol=0, err_msg=k)
    assert 0 < got["precision"] < 1 and 0 < got["recall"] < 1


@pytest.mark.gpu
def test_threshold_is_strict_and_edge_cases():
    gt = PointCloud(torch.tensor([[0.0, 0.0, 0.0], [4.0, 0.0, 0.0]], device=DEV))
    pred = PointCloud(torch.tensor([[0.5, 0.0, 0.0], [4.25, 0.0, 0.0]], device=DEV))   # distances 0.5 and 0.25, exact
    m = mm.mesh_metrics(pred, gt, threshold=0.5)
    assert m["precision"] == 0.5 and m["recall"] == 0.5 and m["acc"] == 0.375 and m["comp"] == 0.375
    m = mm.mesh_metrics(pred, gt, threshold=0.25)
    assert m["precision"] == 0 and m["recall"] == 0 and m["f_score"] == 0
    e = mm.mesh_metrics(PointCloud(torch.zeros((0, 3), device=DEV)), gt)
    assert np.isnan(e["acc"]) and np.isnan(e["precision"]) and e["comp"] == np.inf and e["chamfer"] == np.inf
    assert e["recall"] == 0 and e["f_score"] == 0
    with pytest.raises(ValueError):
        mm.mesh_metrics(pred, PointCloud(torch.zeros((0, 3), device=DEV)))


@pytest.mark.gpu
def test_sampler_matches_oracle():
    mesh = synthetic.raycast_scene_mesh(1, spacing=0.1)
    n = 200_000
    pts, face = mm._sample(mesh, n, seed=7, device=torch.device(DEV))
    v, f = mesh.vertices.numpy(), mesh.faces.numpy().astype(np.int64)
    opts, oface, amb = mo.sample_surface(v, f, n, seed=7)
    got_face = face.cpu().numpy()
    ok = ~amb
    assert amb.mean() < 1e-3
    np.testing.assert_array_equal(got_face[ok], oface[ok])
    np.testing.assert_array_equal(pts.cpu().numpy()[ok], opts[ok])
    # on its triangle: barycentric residual
    P = pts.cpu().numpy().astype(np.float64)
    a, b, c = (v[f[got_face, k]].astype(np.float64) for k in range(3))
    e1, e2, r = b - a, c - a, P - a
    G = np.stack([np.stack([(e1 * e1).sum(1), (e1 * e2).sum(1)], 1), np.stack([(e1 * e2).sum(1), (e2 * e2).sum(1)], 1)], 1)
    lam = np.linalg.solve(G, np.stack([(r * e1).sum(1), (r * e2).sum(1)], 1)[..., None])[..., 0]
    resid = np.linalg.norm(a + lam[:, :1] * e1 + lam[:, 1:] * e2 - P, axis=1)
    assert resid.max() <= 1e-6
    assert (lam >= -1e-5).all() and (lam.sum(1) <= 1 + 1e-5).all()
    # chi-square of per-face counts against areas, faces pooled into 200 groups of similar expected counts
    cr = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]]).astype(np.float64)
    area = 0.5 * np.linalg.norm(cr, axis=1)
    groups = np.minimum((np.cumsum(area) / area.sum() * 200).astype(np.int64), 199)
    expect = np.bincount(groups, weights=area, minlength=200) / area.sum() * n
    got = np.bincount(groups[got_face], minlength=200)
    chi2 = ((got - expect) ** 2 / expect).sum()
    assert chi2 < 199 + 6 * np.sqrt(2 * 199)
    assert area[got_face].min() > 0
    # identical bits on a second run, different points with another seed
    pts2, _ = mm._sample(mesh, n, seed=7, device=torch.device(DEV))
    assert torch.equal(pts, pts2)
    pts3 = mm.sample_surface(mesh, n, seed=8, device=torch.device(DEV)).points
    assert not torch.equal(pts, pts3)
    with pytest.raises(ValueError):
        flat = TriangleMesh(torch.zeros(3, 3), torch.tensor([[0, 1, 2]], dtype=torch.int32))
        mm.sample_surface(flat, 10, device=torch.device(DEV))
    with pytest.raises(ValueError):
        mm.sample_surface(TriangleMesh(mesh.vertices, mesh.faces + 10 ** 7), 10, device=torch.device(DEV))


@pytest.mark.gpu
@pytest.mark.parametrize("sampling", ["vertices", "surface"])
def test_mesh_metrics_deterministic(sampling):
    gt = synthetic.raycast_scene_mesh(0, spacing=0.05)
    pred = TriangleMesh(gt.vertices + 0.01 * torch.sin(gt.vertices * 7), gt.faces)
    a = mm.mesh_metrics(pred, gt, sampling=sampling, n_points=100_000, device=DEV)
    b = mm.mesh_metrics(pred, gt, sampling=sampling, n_points=100_000, device=DEV)
    assert a == b
    assert a["precision"] > 0.5 and a["acc"] < 0.05


def _fuse_scene(tmp_path, noise, N=126, h=160, w=96):
    """raycast_scene over a full loop of the camera path (126 frames of 0.05 rad), portrait frames for an 85 degree
    vertical field of view, fused by OurFuser with the volume sized from the ground-truth mesh (gt_path: read_ply and
    TSDF.from_mesh).  Returns the scene, the ground truth, its path, the fused mesh and the fuser's volume."""
    sc = synthetic.raycast_scene(N, h, w, seed=0, noise=noise, device=DEV)
    gt = synthetic.raycast_scene_mesh(0)
    gt_path = str(tmp_path / "gt.ply")
    gt.write_ply(gt_path)
    fuser = OurFuser(gt_path=gt_path, fusion_resolution=0.04, max_fusion_depth=5.0, device=DEV)
    K = torch.eye(4, device=DEV).repeat(N, 1, 1)
    K[:, :3, :3] = sc["K"]
    for s in range(0, N, 8):
        fuser.fuse_frames(sc["depths"][s:s + 8].unsqueeze(1), K[s:s + 8], sc["cam_T_world"][s:s + 8])
    return sc, gt, gt_path, fuser.get_mesh(), fuser.tsdf_fuser_pred.tsdf


def _observed_vertices(mesh, vol):
    """The mesh vertices whose edge joins two observed voxels (weight > 0).  The reference's fuser has no weight mask,
    so the boundary between observed free space (+1) and never-observed voxels (-1) is meshed too; on this camera
    path (every camera looks along the loop) that frontier is a large part of the mesh, and it is not the surface."""
    u = (mesh.vertices - vol.origin.float().to(DEV)) / vol.voxel_size
    lo, hi = torch.floor(u + 1e-3).long(), torch.ceil(u - 1e-3).long()
    dims = torch.tensor(vol.tsdf_weights.shape, device=DEV)
    ok = ((lo >= 0) & (hi < dims)).all(1)
    lo, hi = torch.minimum(lo.clamp(min=0), dims - 1), torch.minimum(hi.clamp(min=0), dims - 1)
    wts = vol.tsdf_weights
    ok &= (wts[lo[:, 0], lo[:, 1], lo[:, 2]] > 0) & (wts[hi[:, 0], hi[:, 1], hi[:, 2]] > 0)
    return PointCloud(mesh.vertices[ok].contiguous()).voxel_down_sample(0.02)


@pytest.mark.gpu
def test_fusion_scored_against_analytic_ground_truth(tmp_path):
    """Measured on an MI355X (fusion and scoring are deterministic, so these repeat bit for bit): observed vertices,
    noise-free / noise 0.02, precision 0.947 / 0.912, acc 0.0141 / 0.0225 m, f_score 0.859 / 0.846; the whole mesh
    recall 0.923, comp 0.025 m (precision 0.31: the frontier), surface protocol recall 0.81; the downsampled point cloud
    precision 1.0, acc 0.0096 m.  The bounds leave a margin of about 5 % (precision) to 40 % (distances)."""
    sc, gt, gt_path, mesh, vol = _fuse_scene(tmp_path, 0.0)
    whole = mm.mesh_metrics(mesh, gt_path)
    clean = mm.mesh_metrics(_observed_vertices(mesh, vol), gt)
    _, _, _, noisy_mesh, noisy_vol = _fuse_scene(tmp_path, 0.02)
    noisy = mm.mesh_metrics(_observed_vertices(noisy_mesh, noisy_vol), gt)
    pc, _ = point_cloud.fuse_scene(sc["depths"], sc["images"], sc["cam_T_world"], sc["K"])
    pcm = mm.mesh_metrics(pc.voxel_down_sample(0.02), gt)
    surf = mm.mesh_metrics(mesh, gt, sampling="surface")
    print("\nmesh_metrics whole", json.dumps(whole), "\nclean", json.dumps(clean), "\nnoisy", json.dumps(noisy),
          "\npoint cloud", json.dumps(pcm), "\nsurface", json.dumps(surf))
    assert whole["recall"] >= 0.85 and whole["comp"] <= 0.04
    assert clean["precision"] >= 0.9 and clean["acc"] <= 0.02
    assert noisy["acc"] > clean["acc"] and noisy["f_score"] < clean["f_score"]
    assert pcm["precision"] >= 0.95 and pcm["acc"] <= 0.015
    assert surf["recall"] >= 0.7


@pytest.mark.gpu
def test_evaluate_writes_mesh_metrics(tmp_path):
    from simplerecon_amd import depth_model as dm
    from simplerecon_amd.evaluation import evaluate
    from test_gpu_metrics import _frames
    K, h, w = 3, 32, 48
    opts = dm.default_options(image_width=2 * w, image_height=2 * h, model_num_views=K + 1, matching_num_depth_bins=8)
    model = dm.DepthModel(opts)
    for i, m in enumerate((model.encoder, model.matching_model, model.cost_volume_net, model.depth_decoder,
                           model.cost_volume.mlp)):
        synthetic.seeded_fill_(m, seed=21 + i)
    model = model.to(DEV).eval()
    scans = [("scene_a", _frames(4, K, h, w, seed=1)), ("scan/b", _frames(2, K, h, w, seed=2))]
    gt = synthetic.raycast_scene_mesh(0, spacing=0.05)
    bounds = dict(xmin=-3.0, xmax=3.0, ymin=-2.0, ymax=2.0, zmin=-3.0, zmax=3.0)
    evaluate(model, scans, str(tmp_path), "synthetic", batch_size=2, run_fusion=True,
             fuser_factory=lambda scan: OurFuser(bounds=bounds, device=DEV), gt_mesh_factory=lambda scan: gt)
    scores = tmp_path / "scores"
    assert sorted(os.listdir(scores)) == sorted([
        "all_frame_avg_metrics_test.json", "all_scene_avg_metrics_test.json", "scan_b_metrics.json",
        "scene_a_metrics.json", "scan_b_mesh_metrics.json", "scene_a_mesh_metrics.json",
        "all_scene_avg_mesh_metrics_test.json"])
    per_scene = []
    for scan in ("scene_a", "scan_b"):
        mesh_path = next((tmp_path / "meshes").rglob(f"{scan}.ply"))
        want = mm.mesh_metrics(str(mesh_path), gt, device=DEV)
        data = json.load(open(scores / f"{scan}_mesh_metrics.json"))
        assert list(data["scores"]) == list(mm.METRIC_KEYS)
        for k in mm.METRIC_KEYS:
            assert data["scores"][k] == want[k] or (np.isnan(want[k]) and np.isnan(data["scores"][k]))
        per_scene.append(want)
    avg = json.load(open(scores / "all_scene_avg_mesh_metrics_test.json"))["scores"]
    for k in mm.METRIC_KEYS:
        np.testing.assert_allclose(avg[k], np.mean([s[k] for s in per_scene]), rtol=1e-15)
