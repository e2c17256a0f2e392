"""Whole pipelines with every `torch.empty` / `torch.empty_like` result arriving poisoned (hostile_memory.poisoned_empty):
outputs, concat buffers whose sibling slices are still unwritten, workspaces, counters and masks all start as 0xFF bytes in
one run and as 0x7F bytes in another.  Production allocates all of them with torch.empty; a fresh process mostly hands out
zeros, which is often exactly the value an element nobody wrote should have had.

Each pipeline runs twice unpoisoned on fresh objects, then once under each pattern on fresh objects (cached workspaces
dropped).  An output on which the two unpoisoned runs agree bit for bit must come out with the same bits under poison.  An
output that differs between the two unpoisoned runs is summed with atomics; it must be declared in `loose` with the
tolerance its own parity test holds it to (so is a declared output of fewer than 64 elements, which can agree between two
runs by chance).  That tolerance is only the ceiling of its bound: the parity tests measure a kernel against another
computation, here two runs of the SAME computation are compared, which differ by the order of their atomic sums alone.  The
two unpoisoned runs measure that difference; a poisoned run may differ from them by no more than NOISE_FACTOR times the
largest difference any declared output of the pipeline showed, or NOISE_FACTOR times the pipeline's `resolution` if that is
more: one ulp of the narrowest format it rounds to (fp32, or the autocast dtype).  Two runs are a small sample: a reordered
fp32 sum either flips the rounding of a value stored in that format or it does not, and a flip moves the value by one ulp,
whether or not the first two runs happened to show one.  A poison value that reaches a result (NaN, 3.4e38) moves it by many
orders of magnitude more.  Outputs are finite exactly where the unpoisoned ones are."""
import numpy as np
import pytest
import torch

from hostile_memory import PATTERNS, bits, poisoned_empty
from simplerecon_amd import depth_model as dm
from simplerecon_amd import ops, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHANCE_NUMEL = 64   # below this many elements, two atomics-ordered sums can come out equal twice in a row
NOISE_FACTOR = 8    # a third sample of the run-to-run difference against the largest of the first samples; several flips add up
ULP32 = torch.finfo(torch.float32).eps


def _flat(out, prefix=""):
    """{name: tensor} of everything tensor-like in a nested result (floats become 0-dim float64 tensors)."""
    flat = {}
    if isinstance(out, torch.Tensor):
        flat[prefix or "out"] = out.detach()
    elif isinstance(out, dict):
        for k, v in out.items():
            flat.update(_flat(v, f"{prefix}{k}."))
    elif isinstance(out, (list, tuple)):
        for i, v in enumerate(out):
            flat.update(_flat(v, f"{prefix}{i}."))
    elif isinstance(out, (float, int, np.floating, np.integer)) and not isinstance(out, bool):
        flat[prefix or "out"] = torch.tensor(float(out), dtype=torch.float64)
    return flat


def _range_rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) if a.numel() else 0.0


def check_pipeline(make, what, loose=None, metric=_range_rel, resolution=ULP32):
    """`make()` builds fresh objects, runs the pipeline and returns its outputs.  `loose`: {output-name prefix: tolerance} for
    the outputs that atomics make irreproducible; `resolution`: one ulp (relative) of the narrowest format the pipeline rounds
    intermediate values to."""
    loose = loose or {}
    ops._WORKSPACES.clear()
    runs = [_flat(make()), _flat(make())]
    for pattern in PATTERNS:
        ops._WORKSPACES.clear()
        with poisoned_empty(pattern):
            runs.append(_flat(make()))
        torch.cuda.synchronize()
    ops._WORKSPACES.clear()
    a, b = runs[0], runs[1]
    assert a and all(set(r) == set(a) for r in runs), [sorted(r) for r in runs]
    tols = {k: next((t for p, t in loose.items() if k.startswith(p)), None) for k in a}
    fins = {k: torch.isfinite(a[k]) if a[k].is_floating_point() else torch.ones_like(a[k], dtype=torch.bool) for k in a}
    # the run-to-run difference of this pipeline: the largest over its declared outputs
    level = max([metric(b[k][fins[k]], a[k][fins[k]]) for k in a if tols[k] is not None and b[k].shape == a[k].shape] + [resolution])
    compared = 0
    for k in a:
        reproducible = a[k].shape == b[k].shape and bool((bits(a[k]) == bits(b[k])).all())
        tol = tols[k]
        assert reproducible or tol is not None, f"{what}: `{k}` differs between two unpoisoned runs and is not declared loose"
        for pattern, r in zip(PATTERNS, runs[2:]):
            tag = f"{what}: `{k}` under {pattern:#04x}"
            assert r[k].shape == a[k].shape and r[k].dtype == a[k].dtype, tag
            if a[k].is_floating_point():
                assert torch.equal(torch.isfinite(r[k]), torch.isfinite(a[k])), f"{tag}: finite where the unpoisoned run is not, or the reverse"
            same = bits(r[k]) == bits(a[k])
            # (a declared-loose tensor of a few elements -- the bias gradient of a one-channel head -- can agree between two
            # runs by chance: two equal unpoisoned runs do not prove it reproducible)
            if reproducible and not (tol is not None and a[k].numel() < CHANCE_NUMEL):
                assert bool(same.all()), f"{tag}: {int((~same).sum())} of {same.numel()} elements differ from the unpoisoned runs"
            elif not bool(same.all()):
                fin, bound = fins[k], min(tol, NOISE_FACTOR * level)
                err, noise = metric(r[k][fin], a[k][fin]), metric(b[k][fin], a[k][fin])
                print(f"{tag}: {err:.2e} from the unpoisoned run (two unpoisoned runs: {noise:.2e} here, {level:.2e} at most; "
                      f"bound {bound:.1e})")
                assert err <= bound, f"{tag}: {err:.3e} > {bound:.1e} = min({tol:.0e}, {NOISE_FACTOR} x {level:.2e})"
            compared += 1
    print(f"{what}: {len(a)} outputs, {compared} comparisons, run-to-run difference (or resolution) {level:.2e}, "
          f"{sum(1 for k in a if not bool((bits(a[k]) == bits(b[k])).all()))} not bit-reproducible")


# ---- the depth model ------------------------------------------------------------------------------------------------------

def _model(h, w, K, D, train=False):
    opts = dm.default_options(image_width=4 * w, image_height=4 * h, model_num_views=K + 1, matching_num_depth_bins=D)
    model = dm.DepthModel(opts)
    synthetic.seeded_fill_(model.encoder, seed=9, gain=1.0)
    for i, m in enumerate((model.matching_model, model.cost_volume_net, model.depth_decoder, model.cost_volume.mlp)):
        synthetic.seeded_fill_(m, seed=10 + i)
    model = model.to(DEV)
    return model.train() if train else model.eval()


def _inputs(B, K, h, w, seed):
    inp = {k: v.to(DEV) for k, v in synthetic.cost_volume_inputs(B, K, 16, h, w, seed=seed).items()}
    g = torch.Generator(device="cpu").manual_seed(seed)
    cur = torch.randn((B, 3, 4 * h, 4 * w), generator=g).to(DEV)
    src = torch.randn((B, K, 3, 4 * h, 4 * w), generator=g).to(DEV)
    return cur, src, inp["src_extrinsics"], inp["src_poses"], inp["src_Ks"], inp["cur_invK"]


@pytest.mark.parametrize("streams", [1, 2])
def test_forward_tensors(streams):
    """The test_gpu_graph.py shape (96 x 128 image, K = 2, D = 8), the image-prior encoder on its side stream; with two
    sub-batch streams at batch 2.  Decoder and CVEncoder write channel slices of torch.empty concat buffers."""
    B, K, D, h, w = streams, 2, 8, 24, 32
    a = _inputs(B, K, h, w, 3)

    def make():
        model = _model(h, w, K, D)
        model.prior_on_side_stream = True
        model.num_streams = streams
        with torch.inference_mode():
            out = model.forward_tensors(*a, return_mask=True)
            torch.cuda.synchronize()
            return {k: v.clone() for k, v in out.items() if v is not None}
    check_pipeline(make, f"forward_tensors, {streams} stream(s)")


def _training_step(what, dt=None, tol=1e-4):
    """`DepthModel.step("train", ...)` and its backward pass at the test_gpu_training_losses.py shape: both encoders, the MLP
    plane sweep, CVEncoder, decoder, normals and the loss cocktail; the loss and every parameter gradient are compared.
    `dt`: the same step inside torch.autocast(dt) + experimental.autocast_mfma16(mode=2), which turns on HALF_IO, STORE_HALF and
    MFMA16 = 2 (fp16 with the loss scaled by 2^10 and the gradients divided back, as a loss scaler does)."""
    import contextlib
    from simplerecon_amd import autograd_ops, experimental
    B, K, h, w = 2, 3, 32, 48
    scale = 2.0 ** 10 if dt == torch.float16 else 1.0
    floor = {}

    def make():
        opts = dm.default_options(image_width=2 * w, image_height=2 * h, model_num_views=K + 1, matching_num_depth_bins=8)
        model = dm.DepthModel(opts)
        for i, m in enumerate((model.encoder, model.matching_model, model.cost_volume_net, model.depth_decoder,
                               model.cost_volume.mlp)):
            synthetic.seeded_fill_(m, seed=11 + i)
        model = model.to(DEV).train()
        cur, src = synthetic.training_batch(B, K, h, w, seed=6, device=DEV)
        torch.manual_seed(0)
        with contextlib.ExitStack() as stack:
            if dt is not None:
                stack.enter_context(experimental.autocast_mfma16(mode=2))
                assert (autograd_ops.HALF_IO, autograd_ops.STORE_HALF, autograd_ops.MFMA16) == (True, True, 2)
            with torch.autocast("cuda", dtype=dt, enabled=dt is not None):
                loss = model.step("train", (cur, src))
            (loss * scale).backward()          # inside the mfma16 block: the data gradient reads the switch
        torch.cuda.synchronize()
        grads = {n: p.grad / scale for n, p in model.named_parameters() if p.grad is not None}
        assert len(grads) > 100 and sum(bool((g != 0).any()) for g in grads.values()) > 0.9 * len(grads)   # nothing underflowed
        floor["v"] = 1e-3 * max(float(g.abs().max()) for g in grads.values())
        return {"loss": loss.detach().float(), "grad": grads}

    def metric(r, a):
        # a gradient that is zero up to rounding (a bias ahead of a normalisation) has no scale of its own: as in
        # test_gpu_training_losses.py it is measured against 1e-3 of the model's largest gradient
        r, a = r.double(), a.double()
        return float((r - a).abs().max()) / max(float(a.abs().max()), floor["v"]) if a.numel() else 0.0
    check_pipeline(make, what, loose={"grad.": tol, "loss": 1e-6 if dt is None else tol}, metric=metric,
                   resolution=torch.finfo(dt or torch.float32).eps)


def test_training_step_fp32():
    """forward("train"), normals, losses, backward (the test_gpu_training_losses.py shape).  Gradients that the backward kernels
    scatter with atomics: at most that test's bound for parameter gradients (1e-4 of the tensor's largest gradient, floored
    at 1e-3 of the model's largest), and within the run-to-run difference (check_pipeline)."""
    _training_step("fp32 training step")


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=str)
def test_training_step_16bit_autocast(dt):
    """The SAME step as test_training_step_fp32 -- whole model, losses, backward, the loss and every parameter gradient --
    under torch.autocast with 16-bit kernel I/O, 16-bit saved activations and the 16-bit MFMA convolutions on every layer
    that supports them.  The ceiling is the bound test_gpu_half_io.py / test_gpu_conv16.py hold this configuration to (3e-2 fp16,
    2e-1 bf16); what binds is NOISE_FACTOR times the run-to-run difference of the 16-bit step itself or times one ulp of the
    autocast dtype (check_pipeline): 7.8e-3 of a tensor's largest gradient in fp16, 6.2e-2 in bf16, unless the two unpoisoned
    runs differ by more."""
    _training_step(f"16-bit training step {dt}", dt=dt, tol=3e-2 if dt == torch.float16 else 2e-1)


@pytest.mark.parametrize("dt", [torch.float16, torch.bfloat16], ids=str)
def test_conv_stack_16bit_autocast(dt):
    """An extra to the whole-model step: the conv stack alone (CVEncoder -> DepthDecoderPP) on random tensors, the configuration
    and sizes test_gpu_conv16.py trains, where every layer but the heads takes the 16-bit MFMA kernel.  Bounds as above, on
    the relative L2 error."""
    from simplerecon_amd import experimental
    from simplerecon_amd.networks import CVEncoder, DepthDecoderPP
    g = torch.Generator().manual_seed(5)
    B, H, W = 2, 32, 48
    vol0 = torch.randn((B, 16, H, W), generator=g).to(DEV)
    pyr = [torch.randn((B, c, H >> i, W >> i), generator=g).to(DEV) for i, c in enumerate([8, 12, 16, 24])]
    f0 = torch.randn((B, 6, 2 * H, 2 * W), generator=g).to(DEV)

    def make():
        enc = synthetic.seeded_fill_(CVEncoder(16, [8, 12, 16, 24], [16, 24, 32, 48]), seed=1).to(DEV)
        dec = synthetic.seeded_fill_(DepthDecoderPP([6] + enc.num_ch_enc), seed=2).to(DEV)
        vol = vol0.clone().requires_grad_(True)
        with experimental.autocast_mfma16(mode=2):
            with torch.autocast("cuda", dtype=dt):
                out = dec([f0] + enc(vol, pyr))
                loss = sum(out[f"log_depth_pred_s{i}_b1hw"].float().abs().mean() for i in range(4))
            loss.backward()
        torch.cuda.synchronize()
        return {"out": {k: v.detach() for k, v in out.items()}, "loss": loss.detach(), "d_vol": vol.grad,
                "grad": {n: p.grad for m in (enc, dec) for n, p in m.named_parameters() if p.grad is not None}}
    l2 = lambda r, a: float((r.double() - a.double()).norm() / a.double().norm().clamp_min(1e-12))
    tol = 3e-2 if dt == torch.float16 else 2e-1
    check_pipeline(make, f"16-bit conv stack {dt}", loose={"grad.": tol, "d_vol": tol}, metric=l2, resolution=torch.finfo(dt).eps)


# ---- plane sweeps -------------------------------------------------------------------------------------------------------------

def test_dot_cost_volume_forward_and_backward():
    """CostVolumeManager at volume_cases.DOT_SHAPES["spread"]; d src_feats is scattered with atomics (parity.TOL, the bound of
    test_gpu_dot_volume_channels.py run to run)."""
    import volume_cases as vc
    from parity import TOL
    from simplerecon_amd.cost_volume import CostVolumeManager
    shape = vc.DOT_SHAPES["spread"]
    inp = vc.to_device(vc.dot_inputs(shape, 16), DEV)
    cot = torch.from_numpy(vc.cotangent(shape)).to(DEV)

    def make():
        mgr = CostVolumeManager(shape["h"], shape["w"], num_depth_bins=shape["D"], matching_dim_size=16).to(DEV)
        cur, src = inp["cur_feats"].clone().requires_grad_(), inp["src_feats"].clone().requires_grad_()
        vol, lowest, _, _ = mgr(**dict(inp, cur_feats=cur, src_feats=src))
        vol.backward(cot)
        torch.cuda.synchronize()
        return {"vol": vol.detach(), "lowest": lowest, "d_cur": cur.grad, "d_src": src.grad}
    check_pipeline(make, "dot cost volume", loose={"d_src": TOL})


def test_warp_features():
    import volume_cases as vc
    from simplerecon_amd.cost_volume import CostVolumeManager
    case = vc.WARP_CASE
    b, k, c, d, h, w = (case[x] for x in ("B", "K", "C", "D", "h", "w"))
    inp = vc.to_device(vc.inputs(case), DEV)

    def make():
        mgr = CostVolumeManager(h, w, num_depth_bins=d, matching_dim_size=c).to(DEV)
        with torch.inference_mode():
            return [mgr.warp_features(inp["src_feats"], inp["src_extrinsics"], inp["src_Ks"], inp["cur_invK"],
                                      inp["depth_planes_bdhw"][:, j].unsqueeze(1), b, k, c, None) for j in (0, d - 1)]
    check_pipeline(make, "warp_features")


@pytest.mark.parametrize("kind", ["mlp", "dot"])
def test_sweep_workspace_reuse_after_a_larger_call(kind):
    """One manager serves a large call (B = 3, K = 4) and then a small one with another K (B = 1, K = 2): the small call finds
    the large call's records, channels-last sources and packed weights in its workspace.  Its result must equal a fresh
    manager's bit for bit -- with the workspace allocated poisoned, too."""
    from simplerecon_amd.cost_volume import CostVolumeManager, FeatureVolumeManager
    D, h, w = 4, 13, 17

    def manager(K):
        if kind == "dot":
            return CostVolumeManager(h, w, num_depth_bins=D).to(DEV)
        return synthetic.seeded_fill_(FeatureVolumeManager(h, w, num_depth_bins=D, matching_dim_size=16, num_source_views=K), seed=4).to(DEV)
    big = {k: v.to(DEV) for k, v in synthetic.cost_volume_inputs(3, 4, 16, h, w, seed=1).items()}
    small = {k: v.to(DEV) for k, v in synthetic.cost_volume_inputs(1, 2, 16, h, w, seed=2).items()}

    def run(reuse):
        with torch.inference_mode():
            mgr = manager(2)
            if reuse and kind == "dot":
                mgr(**big, return_mask=True)               # the same manager serves both calls, as in production
            elif reuse:
                # the MLP manager's K is a constructor argument (it sizes the MLP's input layer), so the larger call needs a
                # manager of its own: the second one inherits its used, larger workspace
                first = manager(4)
                first(**big, return_mask=True)
                mgr._workspace = first._workspace
            vol, lowest, _, mask = mgr(**small, return_mask=True)
            torch.cuda.synchronize()
            return {"vol": vol, "lowest": lowest, "mask": mask}
    fresh = _flat(run(False))
    for pattern in (None,) + PATTERNS:
        if pattern is None:
            got = _flat(run(True))
        else:
            with poisoned_empty(pattern):
                got = _flat(run(True))
        for k in fresh:
            assert torch.equal(bits(got[k]), bits(fresh[k])), (kind, pattern, k)


# ---- geometry -------------------------------------------------------------------------------------------------------------------

def test_geometry_forward_and_backward():
    from simplerecon_amd.geometry import BackprojectDepth, NormalGenerator, Project3D
    B, h, w = 2, 19, 23
    inp = {k: v.to(DEV) for k, v in synthetic.cost_volume_inputs(B, 2, 16, h, w, seed=5).items()}
    g = torch.Generator().manual_seed(1)
    depth0 = (1.0 + torch.rand((B, 1, h, w), generator=g)).to(DEV)
    cot = torch.randn((B, 3, h, w), generator=g).to(DEV)

    def make():
        depth = depth0.clone().requires_grad_()
        pts = BackprojectDepth(h, w).to(DEV)(depth, inp["cur_invK"])
        pix = Project3D().to(DEV)(pts, inp["src_Ks"][:, 0], inp["src_extrinsics"][:, 0])
        normals = NormalGenerator(h, w).to(DEV)(depth, inp["cur_invK"])
        ((normals * cot).sum() + pix.sum() * 1e-3).backward()
        torch.cuda.synchronize()
        return {"pts": pts.detach(), "pix": pix.detach(), "normals": normals.detach(), "d_depth": depth.grad}
    check_pipeline(make, "geometry", loose={"d_depth": 1e-5})


# ---- scene side -----------------------------------------------------------------------------------------------------------------

def _mesh_dict(mesh):
    return {"v": mesh.vertices, "f": mesh.faces, "n": mesh.normals, "c": mesh.colors}


def test_dense_tsdf_integrate_and_mesh():
    from simplerecon_amd.tsdf import TSDF, TSDFFuser
    sc = synthetic.raycast_scene(4, 40, 56, seed=3, device=DEV)
    K = torch.eye(4, device=DEV).repeat(4, 1, 1)
    K[:, :3, :3] = sc["K"]
    depth, T = sc["depths"][:, None].contiguous().half(), sc["cam_T_world"].half().contiguous()
    bounds = dict(xmin=-2.5, xmax=2.5, ymin=-1.5, ymax=1.5, zmin=-2.5, zmax=2.5)

    def make():
        vol = TSDF.from_bounds(dict(bounds), voxel_size=0.0625, device=DEV)
        fuser = TSDFFuser(vol, max_depth=3.0)
        fuser.integrate_depth(depth[:2], T[:2], K[:2].half())
        fuser.integrate_depth(depth[2:], T[2:], K[2:].half())
        mesh = vol.extract_mesh()
        return {"values": fuser.tsdf_values, "weights": fuser.tsdf_weights, "mesh": _mesh_dict(mesh)}
    check_pipeline(make, "dense TSDF")


def test_sparse_fuser_integrate_and_mesh_with_pool_growth():
    """ScalableTSDFVolume on a ray-cast scene; the second, larger integrate grows the block pool -- the grown pool keeps the
    blocks of the first call and must not read the new allocation's unwritten part."""
    from simplerecon_amd.scalable_tsdf import ScalableTSDFVolume
    N, h, w = 6, 48, 64
    sc = synthetic.raycast_scene(N, h, w, seed=4, device=DEV)
    K = torch.eye(4, device=DEV).repeat(N, 1, 1)
    K[:, :3, :3] = sc["K"]
    depth, T = sc["depths"][:, None].contiguous(), sc["cam_T_world"].contiguous()
    color = sc["images"].permute(0, 3, 1, 2).contiguous()

    def make(capacity=8):
        vol = ScalableTSDFVolume(0.04, 0.12, 3.0, device=DEV, initial_capacity=capacity)
        vol.integrate(depth[:1], K[:1], T[:1], color[:1])
        vol.integrate(depth[1:], K[1:], T[1:], color[1:])
        assert vol.capacity > 8 if capacity == 8 else vol.capacity == capacity   # grown / never grown
        mesh = vol.extract_mesh()
        return {"keys": vol.keys, "tsdf": vol.tsdf, "weights": vol.weights, "colors": vol.colors, "mesh": _mesh_dict(mesh)}
    check_pipeline(make, "sparse TSDF")
    # the pool that grew (under poison) holds what a pool that never had to grow holds
    roomy = _flat(make(1 << 14))
    with poisoned_empty(0xFF):
        grown = _flat(make())
    for k in roomy:
        assert torch.equal(bits(grown[k]), bits(roomy[k])), k


def test_point_cloud_fusion():
    from simplerecon_amd import point_cloud as pcf
    sc = synthetic.raycast_scene(5, 40, 56, seed=11, noise=0.001)

    def make():
        pts, rgb, valid = pcf.process_scene(sc["depths"], sc["images"], sc["cam_T_world"], sc["K"], 0.04, 2)
        return {"pts": torch.as_tensor(pts), "rgb": torch.as_tensor(rgb), "valid": torch.as_tensor(valid)}
    check_pipeline(make, "point-cloud fusion")


def _scene_mesh_and_cameras(N=3, h=40, w=56, seed=2):
    from simplerecon_amd.tsdf import TriangleMesh
    sc = synthetic.raycast_scene(N, h, w, seed=seed)
    m = synthetic.raycast_scene_mesh(seed=seed, spacing=0.1)
    mesh = TriangleMesh(m.vertices.to(DEV), m.faces.to(DEV))
    K = torch.eye(4).repeat(N, 1, 1)
    K[:, :3, :3] = sc["K"]
    return mesh, K.to(DEV), sc["cam_T_world"].float().to(DEV), h, w


def test_rasterise_and_shade():
    from simplerecon_amd import render
    mesh, K, T, h, w = _scene_mesh_and_cameras()

    def make():
        depth, faces = render.render_depth(mesh, K, T, h, w, return_faces=True)
        f32, u8, d2 = render.render_color(mesh, K, T, h, w, output="both", return_depth=True)
        normals = render.render_normals(mesh, K, T, h, w)
        vis = render.visible_faces(mesh, K, T, h, w)
        return {"depth": depth, "faces": faces, "f32": f32, "u8": u8, "d2": d2, "normals": normals, "vis": vis,
                "vn": render.vertex_normals(mesh)}
    check_pipeline(make, "rasterise + shade")


def test_mesh_metrics():
    from simplerecon_amd import mesh_metrics as mm
    from simplerecon_amd.tsdf import TriangleMesh
    gt = synthetic.raycast_scene_mesh(seed=2, spacing=0.1)
    g = torch.Generator().manual_seed(0)
    pred = TriangleMesh((gt.vertices + 0.02 * torch.randn(gt.vertices.shape, generator=g)).to(DEV), gt.faces.to(DEV))
    gt = TriangleMesh(gt.vertices.to(DEV), gt.faces.to(DEV))

    def make():
        return {"vertices": mm.mesh_metrics(pred, gt), "surface": mm.mesh_metrics(pred, gt, sampling="surface", n_points=5000),
                "nn": mm.nearest_distances(pred.vertices, gt.vertices, return_index=True)}
    check_pipeline(make, "mesh metrics")


def test_depth_metrics():
    from simplerecon_amd import metrics
    g = torch.Generator().manual_seed(3)
    gt = (0.3 + 4.0 * torch.rand((3, 1, 48, 64), generator=g)).to(DEV)
    gt[0, 0, :5] = 0.0
    pred = (gt[:, :, ::2, ::2] * (1.0 + 0.1 * torch.randn((3, 1, 24, 32), generator=g).to(DEV))).contiguous()
    mask = gt > 0.5

    def make():
        return {"block": metrics.score_block(gt, pred), "frames": metrics.score_frames(gt, pred),
                "masked": metrics.masked_depth_metrics(gt[:, :, ::2, ::2].contiguous(), pred, mask[:, :, ::2, ::2].contiguous())}
    check_pipeline(make, "depth metrics")


def test_visualisation():
    from simplerecon_amd import visualization as viz
    g = torch.Generator().manual_seed(4)
    depth = (0.5 + 3.0 * torch.rand((2, 1, 37, 53), generator=g)).to(DEV)
    mask = (torch.rand((2, 1, 37, 53), generator=g) > 0.2).to(DEV)
    normals = torch.nn.functional.normalize(torch.randn((2, 3, 37, 53), generator=g), dim=1).to(DEV)
    color = torch.randn((2, 3, 37, 53), generator=g).to(DEV)

    def make():
        return {"range": viz.value_range(depth, mask), "f32": viz.colormap_image(depth[0], mask[0]),
                "u8": viz.colormap_u8(depth[1], mask[1]), "normals": viz.normals_image(normals), "nu8": viz.normals_u8(normals),
                "color": viz.color_image(color), "cu8": viz.color_u8(color)}
    check_pipeline(make, "visualisation")


def test_frame_preparation_and_colour_jitter():
    from simplerecon_amd import frames
    g = torch.Generator().manual_seed(6)
    img = torch.randint(0, 256, (3, 61, 83, 3), generator=g, dtype=torch.uint8).to(DEV)
    depth = torch.randint(0, 12000, (3, 61, 83), generator=g, dtype=torch.int32).to(DEV)
    params = frames.jitter_params(3, generator=torch.Generator().manual_seed(1))

    def make():
        return {"u8": frames.resize_u8(img, 35, 47, "lanczos"), "f32": frames.prepare_color(img, 35, 47, flip=True),
                "jitter": frames.prepare_color_jittered(img, 35, 47, params, flip=True),
                "jitter_raw": frames.prepare_color_jittered(img, 35, 47, params, normalize=False),
                "depth": frames.prepare_depth(depth, 19, 25)}
    check_pipeline(make, "frame preparation + colour jitter")
