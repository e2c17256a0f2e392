"""The dot-product sweep at the feature widths no other test uses: C = 4, 8, 12, 24, 32 (every test elsewhere runs C = 16,
which has kernels of its own).  Forward: the generic sr_dot_volume_kernel<C> in its three launch shapes (no plane split,
single-wave workgroups spread over grid z, plane groups as waves of one workgroup -- tests/volume_cases.py restates the
rule, tests/test_volume_cases_host.py proves the shapes), sr_pack_nhwc_kernel<C>; backward: sr_dot_volume_bwd_kernel<C>,
whose scatter leaves the last lanes of a wave idle at C = 12 and 24; warp_features at C = 8.

Bars: the forward is as close to oracle.dot_volume in float64 as twice the fp32 oracle is (floor 1e-6, never looser than
parity.TOL) -- a bar measured on the reference, the factor 2 for a different but legitimate fp32 summation order; argmax by
parity.assert_lowest_cost, mask exact; gradients against oracle.dot_volume_backward in float64 at 1e-4."""
import numpy as np
import pytest
import torch

import oracle
import volume_cases as vc
from parity import TOL, assert_close, assert_lowest_cost, mismatch_fraction, rel_err
from simplerecon_amd import _lib
from simplerecon_amd.cost_volume import CostVolumeManager
from test_gpu_api_surface import _torch_warp

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _oracle_args(inp):
    n = {k: np.ascontiguousarray(v.numpy()) for k, v in inp.items()}
    return n["cur_feats"], n["src_feats"], n["src_Ks"], n["src_extrinsics"], n["cur_invK"]


def _library_mask(inp, shape, C):
    """sr_dot_volume_fwd with a mask buffer (CostVolumeManager drops the mask, like the reference's dot model)."""
    B, K, D, h, w = (shape[k] for k in ("B", "K", "D", "h", "w"))
    dev = torch.device(DEV)
    ws = torch.empty(_lib.lib().sr_volume_workspace_bytes(B, K, C, h, w), dtype=torch.uint8, device=dev)
    vol = torch.empty((B, D, h, w), device=dev)
    lowest = torch.empty((B, h, w), device=dev)
    mask = torch.full((B, h, w), 7, dtype=torch.uint8, device=dev)
    planes = inp["depth_planes_bdhw"]
    _lib.call("sr_dot_volume_fwd", dev, inp["cur_feats"], inp["src_feats"], inp["src_Ks"], inp["src_extrinsics"],
              inp["cur_invK"], planes, *planes.stride(), B, K, C, h, w, D, vol, D * h * w, h * w, 1, lowest, mask, ws,
              ws.numel())
    torch.cuda.synchronize()
    return vol, lowest, mask


def _forward_case(C, which):
    shape = vc.DOT_SHAPES[which]
    assert vc.dot_launch_shape(shape["B"], shape["h"], shape["w"], shape["D"])[0] == which
    cpu = vc.dot_inputs(shape, C)
    inp = vc.to_device(cpu, DEV)
    mgr = CostVolumeManager(shape["h"], shape["w"], num_depth_bins=shape["D"], matching_dim_size=C).to(DEV)
    with torch.inference_mode():
        vol, lowest, _, none = mgr(**inp)
    torch.cuda.synchronize()
    assert none is None and vol.shape == (shape["B"], shape["D"], shape["h"], shape["w"])
    planes = vc.planes_np(shape, cpu)
    cv32, _, _ = oracle.dot_volume(*_oracle_args(cpu), planes, precision="f32")
    cv64, low64, mask64 = oracle.dot_volume(*_oracle_args(cpu), planes, want_mask=True, precision="f64")
    bar = min(TOL, 2 * max(rel_err(cv32, cv64), 1e-6))
    e = rel_err(vol, cv64)
    print(f"C={C} {which}: HIP vs f64 {e:.3e}, f32 oracle vs f64 {rel_err(cv32, cv64):.3e}, bar {bar:.3e}")
    assert torch.isfinite(vol).all() and e <= bar, (e, bar)
    assert_lowest_cost(lowest, vol, planes, low64, f"C={C} {which}")
    vol2, lowest2, mask = _library_mask(inp, shape, C)
    assert torch.equal(vol2.view(torch.int32), vol.view(torch.int32)) and torch.equal(lowest2, lowest)
    assert mismatch_fraction(mask.bool(), mask64) == 0.0 and int(mask.max()) <= 1


@pytest.mark.parametrize("which", ["nosplit", "spread"])
@pytest.mark.parametrize("C", vc.DOT_CHANNELS)
def test_forward_generic_kernel(C, which):
    _forward_case(C, which)


@pytest.mark.parametrize("C", vc.DOT_WORKGROUP_CHANNELS)
def test_forward_generic_kernel_workgroup_form(C):
    _forward_case(C, "workgroup")


def _grads(mgr, inp, R):
    cur = inp["cur_feats"].clone().requires_grad_()
    src = inp["src_feats"].clone().requires_grad_()
    vol = mgr(**dict(inp, cur_feats=cur, src_feats=src))[0]
    vol.backward(gradient=R)
    torch.cuda.synchronize()
    return cur.grad, src.grad


def _backward_case(C, shape):
    cpu = vc.dot_inputs(shape, C)
    inp = vc.to_device(cpu, DEV)
    mgr = CostVolumeManager(shape["h"], shape["w"], num_depth_bins=shape["D"], matching_dim_size=C).to(DEV)
    cot = vc.cotangent(shape)
    R = torch.from_numpy(cot).to(DEV)
    d_cur, d_src = _grads(mgr, inp, R)
    o_cur, o_src = oracle.dot_volume_backward(cot, *_oracle_args(cpu), vc.planes_np(shape, cpu), precision="f64")
    e1 = assert_close(d_cur, o_cur, what=f"C={C} d cur_feats vs oracle")
    e2 = assert_close(d_src, o_src, what=f"C={C} d src_feats vs oracle")
    print(f"C={C}: d_cur {e1:.3e}, d_src {e2:.3e}")
    d_cur2, d_src2 = _grads(mgr, inp, R)
    assert torch.equal(d_cur.view(torch.int32), d_cur2.view(torch.int32))     # registers only; d_src goes through atomics
    assert_close(d_src2, d_src, what=f"C={C} d src_feats run to run")


@pytest.mark.parametrize("C", vc.DOT_CHANNELS)
def test_backward_ragged(C):
    _backward_case(C, vc.DOT_BWD_CASE)


@pytest.mark.parametrize("C", vc.DOT_BWD_EDGE_CHANNELS)
def test_backward_edge_poses_idle_lane_scatter(C):
    assert 64 % C != 0
    _backward_case(C, vc.DOT_BWD_EDGE_CASE)


def test_warp_features_eight_channels():
    case = vc.WARP_CASE
    b, k, c, d, h, w = (case[x] for x in ("B", "K", "C", "D", "h", "w"))
    cpu = vc.inputs(case)
    inp = vc.to_device(cpu, DEV)
    ref_inp = vc.as_f64(cpu)
    mgr = CostVolumeManager(h, w, num_depth_bins=d, matching_dim_size=c).to(DEV)
    with torch.inference_mode():
        for j in (0, d - 1):
            plane = inp["depth_planes_bdhw"][:, j].unsqueeze(1)
            wp, depths, warped, mask = mgr.warp_features(inp["src_feats"], inp["src_extrinsics"], inp["src_Ks"],
                                                         inp["cur_invK"], plane, b, k, c, None)
            wp_r, depths_r, warped_r, mask_r, _ = _torch_warp(ref_inp, ref_inp["depth_planes_bdhw"][:, j].unsqueeze(1).contiguous(), h, w)
            assert wp.shape == wp_r.shape and warped.shape == (b, k, c, h, w)
            assert_close(wp, wp_r, tol=1e-6, what="world points")
            assert_close(depths, depths_r, tol=1e-5, what="depths")
            assert_close(warped, warped_r, tol=1e-4, what="warped features")
            assert mismatch_fraction(mask, mask_r) < 1e-3
        vol = mgr(**inp)[0]
        dot = ((warped * inp["cur_feats"].unsqueeze(1)).sum(2) * mask).sum(1)
        assert_close(dot, vol[:, d - 1], tol=2e-6, what="warp_features vs fused sweep")
