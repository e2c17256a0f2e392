"""Host side of the training losses (no GPU): the reference's signatures and keys, DepthModel's unchanged state_dict,
the C ABI's declarations, and the refusals of host tensors, non-fp32 inputs and maps smaller than 3x3."""
import inspect

import pytest
import torch

from simplerecon_amd import _lib, geometry, losses, synthetic
from simplerecon_amd import depth_model as dm


def _params(f):
    return list(inspect.signature(f).parameters)


def test_reference_signatures():
    assert _params(losses.MSGradientLoss.__init__) == ["self", "num_scales"]
    assert inspect.signature(losses.MSGradientLoss.__init__).parameters["num_scales"].default == 4
    assert _params(losses.MSGradientLoss.forward) == ["self", "depth_gt", "depth_pred"]
    assert inspect.signature(losses.ScaleInvariantLoss.__init__).parameters["si_lambda"].default == 0.85
    assert _params(losses.ScaleInvariantLoss.forward) == ["self", "log_depth_gt", "log_depth_pred"]
    assert _params(losses.NormalsLoss.forward) == ["self", "normals_gt_b3hw", "normals_pred_b3hw"]
    assert _params(losses.MVDepthLoss.__init__) == ["self", "height", "width"]
    common = ["cur_invK_b44"]
    assert _params(losses.MVDepthLoss.get_valid_mask) == ["self", "cur_depth_b1hw", "src_depth_b1hw", "cur_invK_b44",
                                                          "src_K_b44", "cur_world_T_cam_b44", "src_cam_T_world_b44"]
    assert _params(losses.MVDepthLoss.get_error_for_pair)[:3] == ["self", "depth_pred_b1hw", "cur_depth_b1hw"]
    assert _params(losses.MVDepthLoss.forward) == ["self", "depth_pred_b1hw", "cur_depth_b1hw", "src_depth_bk1hw"] + \
        common + ["src_K_bk44", "cur_world_T_cam_b44", "src_cam_T_world_bk44"]
    sig = inspect.signature(geometry.NormalGenerator.__init__).parameters
    assert list(sig) == ["self", "height", "width", "smoothing_kernel_size", "smoothing_kernel_std"]
    assert sig["smoothing_kernel_size"].default == 5 and sig["smoothing_kernel_std"].default == 2.0
    assert _params(dm.DepthModel.compute_normals) == ["self", "depth_b1hw", "invK_b44"]
    assert _params(dm.DepthModel.compute_losses) == ["self", "cur_data", "src_data", "outputs"]
    assert _params(dm.DepthModel.step) == ["self", "phase", "batch", "batch_idx"]
    with pytest.raises(ValueError):
        geometry.NormalGenerator(8, 8, smoothing_kernel_size=3)
    with pytest.raises(ValueError):
        losses.MSGradientLoss(num_scales=3)


def test_state_dict_prefixes_unchanged_by_the_losses():
    model = dm.DepthModel(dm.default_options(image_width=64, image_height=48, model_num_views=3,
                                             matching_num_depth_bins=8))
    before = list(model.state_dict())
    model._losses_for(24, 32)
    assert list(model.state_dict()) == before
    assert {k.split(".")[0] for k in before} == {"encoder", "cost_volume_net", "depth_decoder", "cost_volume",
                                                 "matching_model"}
    assert not any("loss" in name or "normal" in name for name, _ in model.named_modules())


def test_training_batch_keys():
    cur, src = synthetic.training_batch(2, 3, 12, 16, seed=1)
    for k in ("image_b3hw", "depth_b1hw", "mask_b_b1hw", "mask_b1hw", "K_s0_b44", "invK_s0_b44", "K_s1_b44",
              "invK_s1_b44", "cam_T_world_b44", "world_T_cam_b44"):
        assert k in cur, k
    for k in ("image_b3hw", "depth_b1hw", "K_s0_b44", "cam_T_world_b44", "world_T_cam_b44"):
        assert k in src, k
    assert cur["depth_b1hw"].shape == (2, 1, 12, 16) and src["depth_b1hw"].shape == (2, 3, 1, 12, 16)
    assert cur["image_b3hw"].shape == (2, 3, 24, 32) and cur["mask_b_b1hw"].dtype == torch.bool
    assert torch.isnan(cur["depth_b1hw"]).any() and not cur["mask_b_b1hw"][torch.isnan(cur["depth_b1hw"])].any()


def test_host_tensors_small_maps_and_dtypes_are_refused():
    d = torch.ones((1, 1, 8, 8))
    invK = torch.eye(4)[None]
    with pytest.raises(_lib.HipLibraryError):
        losses.normals_from_depth(d, invK)
    with pytest.raises(_lib.HipLibraryError):
        losses.MSGradientLoss()(d, d)
    with pytest.raises(_lib.HipLibraryError):
        losses.NormalsLoss()(torch.ones((1, 3, 8, 8)), torch.ones((1, 3, 8, 8)))
    with pytest.raises(_lib.HipLibraryError):
        losses.MVDepthLoss(8, 8)(d, d, d[:, None], invK, invK[:, None], invK, invK[:, None])
    with pytest.raises(TypeError):
        losses.MSGradientLoss()(d.double(), d.double())
    with pytest.raises(TypeError):
        losses.ScaleInvariantLoss()(d.half(), d.half())
    lib = _lib.lib()
    assert lib.sr_normals_workspace_bytes(1, 2, 8) == 0 and lib.sr_grad_loss_workspace_bytes(1, 8, 2) == 0
    assert lib.sr_mv_loss_workspace_bytes(1, 16, 8, 8) == 0 and lib.sr_mv_loss_workspace_bytes(1, 15, 8, 8) > 0
    assert lib.sr_normals_workspace_bytes(2, 3, 3) == 8 * 2 * 9 * 4
    # a NULL argument is refused before anything is launched
    assert lib.sr_normals_fwd(None, None, 1, 8, 8, None, None, 0, None) == 1
    assert lib.sr_grad_loss_fwd(None, None, 1, 8, 8, None, None, 0, None) == 1
    with pytest.raises(ValueError):
        geometry.NormalGenerator(2, 8)


def test_header_states_the_filters_and_rules():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                            "simplerecon_hip.h")).read()
    sec = hdr[hdr.index("training losses"):]
    for phrase in ("blur_pool2d(x, 3)", "spatial_gradient(x)", "gaussian_blur2d(x, (5,5), (2,2))", "zero-weight taps",
                   "round half to even", "nanmean", "#define SR_LOSS_MAX_SOURCES 15"):
        assert phrase in sec, phrase
    assert "sr_abi_version" in _lib.SIGNATURES and _lib.ABI_VERSION == 5
