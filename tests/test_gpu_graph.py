"""HIP-graph replay of the step (simplerecon_amd.graph): identical results to eager submission, new inputs are
picked up through the captured buffers."""
import pytest
import torch

from simplerecon_amd import depth_model as dm
from simplerecon_amd import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _model(h, w, K, D):
    opts = dm.default_options(image_width=4 * w, image_height=4 * h, model_num_views=K + 1, matching_num_depth_bins=D)
    model = dm.DepthModel(opts)
    for i, m in enumerate((model.matching_model, model.cost_volume_net, model.depth_decoder, model.cost_volume.mlp)):
        synthetic.seeded_fill_(m, seed=10 + i)
    return model.to(DEV).eval()


def _inputs(B, K, h, w, seed):
    inp = {k: v.to(DEV) for k, v in synthetic.cost_volume_inputs(B, K, 16, h, w, seed=seed).items()}
    pyr = [f.to(DEV) for f in synthetic.image_prior_pyramid(B, h, w, seed=seed)]
    g = torch.Generator(device="cpu").manual_seed(seed)
    cur = torch.randn((B, 3, 4 * h, 4 * w), generator=g).to(DEV)
    src = torch.randn((B, K, 3, 4 * h, 4 * w), generator=g).to(DEV)
    return cur, src, pyr, inp["src_extrinsics"], inp["src_poses"], inp["src_Ks"], inp["cur_invK"]


def test_graphed_step_equals_eager_and_follows_new_inputs():
    B, K, D, h, w = 2, 3, 8, 24, 32
    model = _model(h, w, K, D)
    a, b = _inputs(B, K, h, w, 1), _inputs(B, K, h, w, 2)

    def eager(cur, src, pyr, ext, poses, Ks, invK):
        with torch.inference_mode():
            mc, ms = model.compute_matching_feats(cur, src, False)
            return {k: (v.clone() if v is not None else None) for k, v in
                    model.hot_path(list(pyr), mc, ms, ext, poses, Ks, invK, return_mask=True).items()}
    ref_a, ref_b = eager(*a), eager(*b)
    graphed = model.graphed(*a, return_mask=True)
    for inputs, ref in ((a, ref_a), (b, ref_b), (a, ref_a)):
        out = graphed(*inputs)
        torch.cuda.synchronize()
        assert set(out) == set(ref)
        for k in ref:
            assert torch.equal(out[k], ref[k]), k   # same kernels, same order: bit-identical
    with pytest.raises(ValueError):
        graphed(*(t[:1] if isinstance(t, torch.Tensor) else [f[:1] for f in t] for t in a))


def test_whole_model_graph_with_side_stream_prior_encoder():
    """cur_feats=None: the image-prior encoder (on its side stream) is captured with the rest of forward_tensors."""
    B, K, D, h, w = 1, 2, 8, 24, 32
    opts = dm.default_options(image_width=4 * w, image_height=4 * h, model_num_views=K + 1, matching_num_depth_bins=D)
    model = dm.DepthModel(opts)
    synthetic.seeded_fill_(model.encoder, seed=9, gain=1.0)
    for i, m in enumerate((model.matching_model, model.cost_volume_net, model.depth_decoder, model.cost_volume.mlp)):
        synthetic.seeded_fill_(m, seed=10 + i)
    model = model.to(DEV).eval()
    a, b = _inputs(B, K, h, w, 3), _inputs(B, K, h, w, 4)

    def eager(cur, src, _pyr, ext, poses, Ks, invK, side):
        model.prior_on_side_stream = side
        with torch.inference_mode():
            out = model.forward_tensors(cur, src, ext, poses, Ks, invK, return_mask=True)
            return {k: (v.clone() if v is not None else None) for k, v in out.items()}
    ref_a, ref_b = eager(*a, side=True), eager(*b, side=True)
    same_stream = eager(*a, side=False)
    for k in ref_a:
        assert same_stream[k] is None and ref_a[k] is None or torch.equal(same_stream[k], ref_a[k]), k
    model.prior_on_side_stream = True
    graphed = model.graphed(a[0], a[1], None, *a[3:], return_mask=True)
    for inputs, ref in ((a, ref_a), (b, ref_b), (a, ref_a)):
        out = graphed(inputs[0], inputs[1], None, *inputs[3:])
        torch.cuda.synchronize()
        for k in ref:
            assert torch.equal(out[k], ref[k]), k


def test_sub_batch_streams_equal_single_stream():
    """DepthModel.hot_path with num_streams > 1 runs sub-batches on separate HIP streams through ONE cost-volume
    manager: each stream must get its own sweep workspace (geometry records, channels-last sources, packed MLP) and
    must wait for weights that another stream packed.  Expected value = the same sub-batches run one after the other on
    one stream (bit-identical: a conv launch plan depends on the launch's batch size, so the whole batch in one launch
    may reassociate sums differently and is only compared to tolerance)."""
    B, K, D, h, w = 4, 3, 8, 24, 32
    a = _inputs(B, K, h, w, 5)

    def run(model, lo, hi):
        sl = lambda t: [f[lo:hi] for f in t] if isinstance(t, list) else t[lo:hi]
        mc, ms = model.compute_matching_feats(a[0], a[1], False)   # whole batch, as in the multi-stream call
        return model.hot_path(sl(a[2]), mc[lo:hi], ms[lo:hi], *[sl(t) for t in a[3:]], return_mask=True)

    whole_model = _model(h, w, K, D)       # (models are built outside inference mode: their weights carry versions)
    with torch.inference_mode():
        whole = {k: v.clone() for k, v in run(whole_model, 0, B).items() if v is not None}
    for streams in (2, 4):
        bounds = [(B * i) // streams for i in range(streams + 1)]
        seq_model = _model(h, w, K, D)
        model = _model(h, w, K, D)              # fresh model: weight packing happens inside the multi-stream call
        with torch.inference_mode():
            parts = [run(seq_model, bounds[i], bounds[i + 1]) for i in range(streams)]
            want = {k: torch.cat([p[k] for p in parts], 0) for k in parts[0] if parts[0][k] is not None}
            model.num_streams = streams
            for _ in range(3):                  # repeated calls: workspaces are reused while other streams read theirs
                mc, ms = model.compute_matching_feats(a[0], a[1], False)
                out = model.hot_path(list(a[2]), mc, ms, *a[3:], return_mask=True)
        torch.cuda.synchronize()
        for k in want:
            assert torch.equal(out[k], want[k]), (streams, k)
            if out[k].dtype == torch.float32:
                assert torch.allclose(out[k], whole[k], rtol=1e-4, atol=1e-5), (streams, k)


def test_graph_replay_survives_larger_eager_calls():
    """A captured graph owns its sweep workspace: eager calls with a larger batch afterwards (which grow and replace
    the manager's cached workspace) must not disturb a later replay."""
    K, D, h, w = 3, 8, 24, 32
    model = _model(h, w, K, D)
    a = _inputs(1, K, h, w, 6)
    big = _inputs(6, K, h, w, 7)
    with torch.inference_mode():
        mc, ms = model.compute_matching_feats(a[0], a[1], False)
        ref = {k: v.clone() for k, v in model.hot_path(list(a[2]), mc, ms, *a[3:], return_mask=True).items()}
    graphed = model.graphed(*a, return_mask=True)
    junk = []
    with torch.inference_mode():
        for _ in range(2):
            mc, ms = model.compute_matching_feats(big[0], big[1], False)
            model.hot_path(list(big[2]), mc, ms, *big[3:], return_mask=True)
            junk.append(torch.full((1 << 22,), float("nan"), device=DEV))   # recycle freed blocks with poison
    out = graphed(*a)
    torch.cuda.synchronize()
    for k in ref:
        assert torch.equal(out[k], ref[k]), k


# ---- replay and packed weights ------------------------------------------------------------------------------------------
# The graph bakes in the addresses of the weights packed during warm-up.  They live outside its memory pool; the packed-weight
# cache drops them when a later eager call re-packs.

def _reseeded_state(model, only_conv_weights):
    """A state dict with other values: every floating tensor, or only the convolution weights of CVEncoder and the decoder
    (tensors of which a graph reads the PACKED form only; biases, the sweep's MLP weights and the matching encoder's 1x1
    convolution are read live on every replay)."""
    sd = {}
    for i, (k, v) in enumerate(model.state_dict().items()):
        change = v.is_floating_point() and (not only_conv_weights or (
            v.dim() == 4 and k.startswith(("cost_volume_net.", "depth_decoder."))))
        sd[k] = v * (1.0 + 0.05 * torch.cos(torch.arange(v.numel(), device=v.device, dtype=v.dtype) + i).view(v.shape)) \
            if change and v.dim() > 0 else v.clone()
    return sd


def test_replay_after_a_weight_update_raises():
    from simplerecon_amd import ops
    from simplerecon_amd.graph import StaleGraphError
    K, D, h, w = 2, 8, 24, 32
    model = _model(h, w, K, D)
    a = _inputs(1, K, h, w, 8)
    graphed = model.graphed(*a, return_mask=True, check_weights=True)
    graphed(*a)
    model.load_state_dict(_reseeded_state(model, False))
    with pytest.raises(StaleGraphError, match="[Cc]apture again"):
        graphed(*a)
    graphed = model.graphed(*a, return_mask=True, check_weights=True)      # capturing again is the cure
    with torch.inference_mode():
        mc, ms = model.compute_matching_feats(a[0], a[1], False)
        ref = {k: v.clone() for k, v in model.hot_path(list(a[2]), mc, ms, *a[3:], return_mask=True).items()}
    out = graphed(*a)
    torch.cuda.synchronize()
    for k in ref:
        assert torch.equal(out[k], ref[k]), k
    with torch.no_grad():
        model.depth_decoder.parameters().__next__().mul_(1.5)     # an optimizer-style in-place step
    with pytest.raises(StaleGraphError):
        graphed(*a)
    graphed = model.graphed(*a, return_mask=True)                 # (the check is opt-in; this one is always made)
    ops.forget_packed(model)                                      # what a `.data` writer calls
    with pytest.raises(StaleGraphError, match="forget_packed"):
        graphed(*a)


def test_unchecked_replay_reads_the_weights_it_pinned():
    """check_weights=False: the replay computes with the payloads packed at capture.  New convolution weights + one eager call
    make the cache re-pack and drop its references to the old payloads; junk allocations then recycle whatever was freed, as
    NaN.  The graph holds its own references, so the replay still equals the old-weight result bit for bit.  (Only
    convolution weights of CVEncoder and the decoder change: what a replay reads live follows the module at once.)"""
    K, D, h, w = 2, 8, 24, 32
    model = _model(h, w, K, D)
    a = _inputs(1, K, h, w, 9)

    def eager():
        with torch.inference_mode():
            mc, ms = model.compute_matching_feats(a[0], a[1], False)
            return {k: (v.clone() if v is not None else None)
                    for k, v in model.hot_path(list(a[2]), mc, ms, *a[3:], return_mask=True).items()}
    old = eager()
    graphed = model.graphed(*a, return_mask=True, check_weights=False)
    model.load_state_dict(_reseeded_state(model, True))
    new = eager()                                                 # re-packs every convolution, frees the old payloads
    assert not torch.equal(new["depth_pred_s0_b1hw"], old["depth_pred_s0_b1hw"])
    junk = [torch.full((n,), float("nan"), device=DEV) for n in (1 << 12, 1 << 14, 1 << 16, 1 << 18, 1 << 20, 1 << 22) for _ in range(4)]
    out = graphed(*a)
    torch.cuda.synchronize()
    for k in old:
        assert old[k] is None and out[k] is None or torch.equal(out[k], old[k]), k
    del junk
