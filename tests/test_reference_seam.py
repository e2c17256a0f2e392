"""The drop-in seam against the REAL reference classes, as recorded from them in tests/golden/reference_seam.npz
(tests/golden/make_reference_seam_golden.py runs the reference's own classes on CPU; these tests need nothing outside
the repository).

  * cost_volume.to_hip(reference manager) -- the attribute swap of INTEGRATION.md §1 / reference test.py:196-198 -- for all
    three reference managers: class, (C, K) recovered from the MLP width (reference cost_volume.py:420-435), MLP weights
    and linear_ramp_1d11 carried over, and the twin then runs through the C-ABI (stub library: argument marshalling).
    The manager handed to to_hip is a stand-in with the reference class's name, attributes, state-dict keys and buffer
    values.
  * reference checkpoints load with strict=True: CVEncoder, DepthDecoderPP, ResnetMatchingEncoder, the three managers
    (reference cost_volume.py:58-74, networks.py:20-127, 149-205): our state dicts have the reference's keys, in its
    order, with its shapes and dtypes, and load a state dict of that layout strictly, values included."""
import json
import os

import numpy as np
import pytest
import torch

from simplerecon_amd import cost_volume as cv
from simplerecon_amd import networks as nets
from simplerecon_amd import synthetic
from test_host_logic_stub import stub  # noqa: F401  (fixture)

H, W, D = 12, 16, 8                 # (tests/golden/make_reference_seam_golden.py records the same cases)
ENC_CH = [24, 48, 64, 160, 256]     # EfficientNetV2-S pyramid (reference depth_model.py:110-127)
CV_OUT = [64, 128, 256, 384]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_seam.npz")


@pytest.fixture(scope="module")
def ref():
    with np.load(GOLDEN) as z:
        arrays = {k: z[k] for k in z.files}
    return dict(meta=json.loads(str(arrays.pop("meta"))), arrays=arrays)


def _layout(module):
    return [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in module.state_dict().items()]


def _ref_manager(ref, kind, K):
    """A stand-in for the reference manager: the reference class's name and the attributes to_hip reads, the reference's
    buffers (values as recorded) under their state-dict names, and for the feature-volume managers an MLP of the
    reference's widths -- the module the twin must share."""
    rec = ref["meta"]["managers"][f"{kind}{K}"]
    m = type(rec["class"], (torch.nn.Module,), {})()
    for a, v in rec["attrs"].items():
        setattr(m, a, v)
    for key, _, _ in rec["state_dict"]:
        if key.startswith("mlp."):
            continue
        owner, *path = [m] + key.split(".")[:-1]
        for part in path:
            if not hasattr(owner, part):
                owner.add_module(part, torch.nn.Module())
            owner = getattr(owner, part)
        owner.register_buffer(key.split(".")[-1], torch.from_numpy(ref["arrays"][f"{kind}{K}/{key}"].copy()))
    if "mlp_channels" in rec:
        torch.manual_seed(3)
        m.mlp = nets.MLP(rec["mlp_channels"], disable_final_activation=True)
    return m, rec


@pytest.mark.parametrize("kind,K", [("dot", 3), ("mlp", 7), ("mlp", 2), ("fast", 5)])
def test_to_hip_of_a_reference_manager(ref, stub, kind, K):  # noqa: F811
    m, rec = _ref_manager(ref, kind, K)
    assert _layout(m) == rec["state_dict"]     # the stand-in is the reference manager's state dict
    twin = cv.to_hip(m)
    assert (twin.matching_height, twin.matching_width, twin.num_depth_bins) == (H, W, D)
    assert torch.equal(twin.linear_ramp_1d11, m.linear_ramp_1d11)
    if kind == "dot":
        assert type(twin) is cv.CostVolumeManager and not hasattr(twin, "mlp")
    else:
        assert type(twin) is (cv.FastFeatureVolumeManager if kind == "fast" else cv.FeatureVolumeManager)
        # shared like the reference's own to_fast() (cost_volume.py:739-746): the same module, the same nn.Parameters
        assert twin.mlp is m.mlp
        assert [id(p) for p in twin.mlp.parameters()] == [id(p) for p in m.mlp.parameters()]
        assert (twin.matching_dim_size, twin.num_source_views) == (16, K)          # recovered from the MLP width
        assert twin.mlp_channels == [cv.mlp_input_channels(16, K), 128, 128, 1]
        sd_ref, sd = m.mlp.state_dict(), twin.mlp.state_dict()
        assert list(sd) == list(sd_ref)
        for k in sd:
            assert torch.equal(sd[k], sd_ref[k]), k
    # the twin's state dict has exactly the reference's keys and loads the reference's with strict=True
    assert sorted(twin.state_dict()) == sorted(k for k, _, _ in rec["state_dict"])
    twin.load_state_dict(m.state_dict(), strict=True)
    # ... and it runs (stub library = every C-ABI call checked against the signature table)
    inp = synthetic.cost_volume_inputs(2, K, 16, H, W, seed=1)
    with torch.no_grad():
        vol, lowest, planes, mask = twin(return_mask=True, **inp)
    assert vol.shape == (2, D, H, W) and lowest.shape == (2, H, W) and planes.shape == (2, D, H, W)
    assert ("sr_dot_volume_fwd" if kind == "dot" else "sr_mlp_volume_fwd") in stub
    # depth planes = the reference's own generate_depth_planes
    want = torch.from_numpy(ref["arrays"][f"{kind}{K}/planes"])
    assert torch.allclose(planes, want, rtol=1e-6, atol=0)
    if kind != "dot":
        fast = twin.to_fast()   # the reference's second seam (cost_volume.py:739-746) on our side
        assert isinstance(fast, cv.FastFeatureVolumeManager) and fast.mlp is twin.mlp


def _assert_state_dicts_interchange(ours, layout):
    """`layout` = the reference module's state dict as recorded: keys in order, shapes, dtypes."""
    assert _layout(ours) == layout, (set(k for k, _, _ in _layout(ours)) ^ set(k for k, _, _ in layout))
    rng = np.random.default_rng(11)
    theirs = {k: torch.from_numpy(rng.integers(0, 100, size=shape) if dt == "int64" else
                                  rng.standard_normal(shape).astype(np.float32)).to(getattr(torch, dt))
              for k, shape, dt in layout}
    ours.load_state_dict(theirs, strict=True)
    for k, v in ours.state_dict().items():
        assert torch.equal(v, theirs[k]), k
    # (ours loads into the reference's module strictly as well: the same keys, shapes and dtypes, asserted above)


def test_reference_conv_stack_checkpoints_load_strictly(ref):
    lay = ref["meta"]["layouts"]
    _assert_state_dicts_interchange(nets.CVEncoder(num_ch_cv=D, num_ch_enc=ENC_CH[1:], num_ch_outs=CV_OUT), lay["CVEncoder"])
    _assert_state_dicts_interchange(nets.DepthDecoderPP(ENC_CH[:1] + CV_OUT), lay["DepthDecoderPP"])
    _assert_state_dicts_interchange(nets.MLP([202, 128, 128, 1], disable_final_activation=True), lay["MLP"])


def test_reference_matching_encoder_checkpoint_loads_strictly(ref):
    """Backbone = refshim's restatement of antialiased_cnns.resnet18 (package absent: SURVEY.md §8c); the tail and every
    state-dict key are the reference's (networks.py:163-201)."""
    _assert_state_dicts_interchange(nets.ResnetMatchingEncoder(18, 16).eval(), ref["meta"]["layouts"]["ResnetMatchingEncoder"])


def test_pose_distance_on_host_tensors_matches_the_reference(ref):
    """The reference's dataset workers call pose_distance on CPU poses (generic_mvs_dataset.py:643-659): host tensors take
    the host path and give the reference's values."""
    from simplerecon_amd import geometry
    poses, _ = synthetic.poses(3, 5, seed=2)
    T = torch.from_numpy(poses.reshape(-1, 4, 4))
    ours = geometry.pose_distance(T)
    want = [ref["arrays"][f"pose_distance/{j}"] for j in range(len(ours))]
    assert f"pose_distance/{len(ours)}" not in ref["arrays"]
    for a, b in zip(ours, want):
        assert a.shape == b.shape and not a.is_cuda
        assert np.allclose(a.numpy(), b, rtol=1e-6, atol=1e-7)
