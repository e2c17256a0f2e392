"""DepthModel's training objective end to end on the GPU: forward("train") at a small shape, compute_normals +
compute_losses + backward.  The loss equals the fp64 oracle on the detached outputs, the gradients reaching the
outputs equal the oracle's autograd, and the parameter gradients equal torch.autograd.grad(outputs, params,
oracle_output_grads)."""
import pytest
import torch

import loss_oracle as lo
from simplerecon_amd import depth_model as dm
from simplerecon_amd import synthetic


@pytest.mark.gpu
def test_depth_model_step_losses_and_gradients():
    dev = "cuda"
    B, K, h, w = 2, 3, 32, 48   # depth / prediction at half the image size
    opts = dm.default_options(image_width=2 * w, image_height=2 * h, model_num_views=K + 1, matching_num_depth_bins=8)
    model = dm.DepthModel(opts)
    for i, m in enumerate((model.encoder, model.matching_model, model.cost_volume_net, model.depth_decoder,
                           model.cost_volume.mlp)):
        synthetic.seeded_fill_(m, seed=11 + i)
    model = model.to(dev).train()
    cur, src = synthetic.training_batch(B, K, h, w, seed=6, device=dev)
    torch.manual_seed(0)
    outputs = model("train", cur, src)
    assert outputs["depth_pred_s0_b1hw"].shape == (B, 1, h, w)
    cur["normals_b3hw"] = model.compute_normals(cur["depth_b1hw"], cur["invK_s0_b44"])
    outputs["normals_pred_b3hw"] = model.compute_normals(outputs["depth_pred_s0_b1hw"], cur["invK_s0_b44"])
    losses = model.compute_losses(cur, src, outputs)
    assert set(losses) == set(lo.KEYS)
    keys = ["depth_pred_s0_b1hw"] + [f"log_depth_pred_s{i}_b1hw" for i in range(4)]
    outs = [outputs[k] for k in keys]
    params = [p for p in model.parameters() if p.requires_grad]
    # one backward pass for everything (the graph is traversed once)
    got = torch.autograd.grad(losses["loss"], outs + params, allow_unused=True)
    got_out, got_p = got[:len(outs)], got[len(outs):]

    inputs = {"depth_b1hw": cur["depth_b1hw"].cpu(), "mask_b_b1hw": cur["mask_b_b1hw"].cpu(),
              "invK_s0_b44": cur["invK_s0_b44"].cpu(), "world_T_cam_b44": cur["world_T_cam_b44"].cpu(),
              "src_depth_bk1hw": src["depth_b1hw"].cpu(), "src_K_s0_bk44": src["K_s0_b44"].cpu(),
              "src_cam_T_world_bk44": src["cam_T_world_b44"].cpu()}
    inputs.update({k: v.detach().cpu() for k, v in zip(keys, outs)})
    orc = lo.run(inputs)
    for k in lo.KEYS:
        assert lo.rel_err(losses[k].detach().cpu(), orc["terms"][k]) < 1e-4, k
    amb = orc["mv_ambiguous"].any(1, keepdim=True)
    # the oracle's gradients are partials with respect to each output as a leaf; in the model depth_pred_s0 =
    # exp(log_depth_pred_s0), so what reaches log_depth_pred_s0 also carries the depth_pred_s0 path
    direct = {k: orc["grads"][f"loss/{k}"] for k in keys}
    total = dict(direct)
    total["log_depth_pred_s0_b1hw"] = direct["log_depth_pred_s0_b1hw"] + \
        direct["depth_pred_s0_b1hw"] * inputs["depth_pred_s0_b1hw"].double()
    for k, g in zip(keys, got_out):
        keep = ~amb if k in ("depth_pred_s0_b1hw", "log_depth_pred_s0_b1hw") else torch.ones_like(total[k], dtype=torch.bool)
        assert lo.rel_err(torch.where(keep, g.double().cpu(), total[k]), total[k]) < 5e-4, k
    # parameter gradients: the network's backward fed with the oracle's output gradients
    # on a fresh forward graph of the same batch (same seed: same flip)
    torch.manual_seed(0)
    outputs2 = model("train", cur, src)
    outs2 = [outputs2[k] for k in keys]
    assert all(torch.equal(a.detach(), b.detach()) for a, b in zip(outs, outs2))
    orc_p = torch.autograd.grad(outs2, params, grad_outputs=[direct[k].float().to(dev) for k in keys],
                                allow_unused=True)
    # Each tensor's error is taken relative to its largest gradient, floored at 1e-3 of the largest parameter gradient
    # of the model: some parameters (biases ahead of a normalisation) have a gradient that is zero up to rounding.
    assert all((a is None) == (b is None) for a, b in zip(got_p, orc_p))
    pairs = [(a.double().cpu(), b.double().cpu()) for a, b in zip(got_p, orc_p) if a is not None]
    top = max(float(b.abs().max()) for _, b in pairs)
    worst = max(float((a - b).abs().max()) / max(float(b.abs().max()), 1e-3 * top) for a, b in pairs)
    # pixels with an ambiguous multi-view decision (if any) are part of these sums
    assert worst < (1e-3 if bool(amb.any()) else 1e-4), worst
    # step(): forward, normals, losses -> the scalar loss, differentiable in the parameters
    loss = model.step("train", synthetic.training_batch(B, K, h, w, seed=6, device=dev))
    assert loss.dim() == 0 and loss.requires_grad and bool(torch.isfinite(loss))
