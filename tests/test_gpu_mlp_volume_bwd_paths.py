"""The paths of the metadata-MLP sweep's backward (csrc/sr_mlp_volume_bwd.hip) that tests/test_gpu_mlp_volume_bwd.py does
not reach, each against oracle.mlp_volume_backward in float64 at the project's backward bar (parity.assert_close, 1e-4
range-relative) on all eight gradients and the forward under autograd:

  * the persistent loop: more work items than CUs, so workgroups take a second (image, 32-pixel tile) item with the dW1 /
    dW2 accumulators live, at K = 2 and at K = 7 (Cin = 202), ragged last tile (tests/volume_cases.py; cotangents zeroed
    on LeakyReLU kinks, proven sufficient from the oracle alone in tests/test_volume_cases_host.py);
  * view counts 1, 4, 5, 9, 11, 12: all four dW1 instantiations (NT1 = 4 / 7 / 10 / 13), K = 5 with unused column tiles;
  * edge poses (a view behind the camera, mostly out-of-bounds samples, identity) and per-pixel depth planes;
  * cotangent layouts: contiguous, channels-last, a row-padded view (the .contiguous() branch), the stride-0 gradient of
    vol.sum();  batch 3 with image independence and run-to-run bit equality of d_cur_feats (no atomics on that path);
  * a frozen MLP.

Measured errors of a run are written to $SR_VOLUME_PARITY_OUT (json) when that variable is set
(profiles/volume_bwd_parity.json)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import volume_cases as vc
from parity import TOL, rel_err
from simplerecon_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = {"net.0.weight": "dW1", "net.0.bias": "db1", "net.2.weight": "dW2", "net.2.bias": "db2", "net.4.weight": "dW3",
         "net.4.bias": "db3"}
MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_measured():
    yield
    path = os.environ.get("SR_VOLUME_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"metric": "parity.rel_err of the HIP backward of the metadata-MLP sweep against "
                                 "oracle.mlp_volume_backward(precision='f64') (max|a-b| / max|b|), bound 1e-4",
                       "cases": MEASURED}, f, indent=1, sort_keys=True)


def _check(case_id, what, got, want, tol=TOL):
    e = rel_err(got, want)
    MEASURED.setdefault(case_id, {})[what] = e
    print(f"{case_id}: {what} rel err {e:.3e} (bound {tol:.0e})")
    assert torch.isfinite(got).all(), f"{case_id}: {what} has non-finite values"
    assert e <= tol, f"{case_id}: {what} rel err {e:.3e} > {tol:.1e}"


def _run(mgr_cpu, inp_cpu, cot, frozen=False):
    """One forward + backward on the device -> (volume, {gradient name: tensor}, manager).  cot: a device tensor of any
    layout, or None for vol.sum().backward()."""
    mgr = copy.deepcopy(mgr_cpu).to(DEV)
    if frozen:
        mgr.mlp.requires_grad_(False)
    inp = vc.to_device(inp_cpu, DEV)
    cur = inp["cur_feats"].clone().requires_grad_()
    src = inp["src_feats"].clone().requires_grad_()
    vol, lowest, _, mask = mgr(**dict(inp, cur_feats=cur, src_feats=src), return_mask=True)
    assert vol.requires_grad and not lowest.requires_grad and mask.dtype == torch.bool
    if cot is None:
        vol.sum().backward()
    else:
        vol.backward(gradient=cot)
    torch.cuda.synchronize()
    grads = {"d_cur_feats": cur.grad, "d_src_feats": src.grad}
    for k, prm in mgr.mlp.named_parameters():
        grads[NAMES[k]] = prm.grad
    return vol.detach(), grads, mgr


def _check_all(case_id, vol, grads, fwd, ref, keys=vc.GRAD_KEYS):
    _check(case_id, "forward", vol, fwd)
    for key in keys:
        _check(case_id, key, grads[key], ref[key])


def _small_reference(case, cot):
    inp, mgr = vc.inputs(case), vc.manager(case)
    mlp = vc.mlp_dict(mgr)
    return inp, mgr, vc.oracle_forward(case, inp, mlp), vc.oracle_backward(case, inp, mlp, cot)


@pytest.mark.parametrize("name", [c["name"] for c in vc.PERSISTENT_CASES])
def test_persistent_loop_second_work_item(name):
    case = next(c for c in vc.PERSISTENT_CASES if c["name"] == name)
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    items = vc.mlp_bwd_items(case["B"], case["h"], case["w"])
    if items <= cus:
        pytest.skip(f"{name}: {items} work items on {cus} CUs -- no workgroup would take a second item on this device")
    assert items > cus
    ref = vc.at_size_reference(name)
    assert ref["share"] <= vc.KINK_SHARE_MAX and ref["agree"] <= vc.ORACLE_AGREE_MAX, (ref["share"], ref["agree"])
    vol, grads, _ = _run(ref["mgr"], ref["inp"], torch.from_numpy(ref["cot"]).to(DEV))
    _check_all(name, vol, grads, ref["fwd"], ref["ref"])


@pytest.mark.parametrize("case", vc.VIEW_CASES + [vc.EDGE_CASE, vc.PIXEL_PLANES_CASE], ids=lambda c: c["name"])
def test_view_counts_edge_poses_and_pixel_planes(case):
    cot = vc.cotangent(case)
    inp, mgr, fwd, ref = _small_reference(case, cot)
    if case.get("pixel_planes"):
        assert vc.planes_np(case, inp).ndim == 4 and float(inp["depth_planes_bdhw"][0, 0].std()) > 0.0
    vol, grads, dmgr = _run(mgr, inp, torch.from_numpy(cot).to(DEV))
    assert dmgr.mlp.net[0].in_features == vc.mlp_cin(case["K"])
    _check_all(case["name"], vol, grads, fwd, ref)


def test_cotangent_layouts(monkeypatch):
    """The strides the backward hands to the library are recorded: (b, d, x) strides of the dense layouts as they are, a
    row-padded view through .contiguous(), the expanded gradient of vol.sum() with all strides zero."""
    case = vc.LAYOUT_CASE
    B, D, h, w = case["B"], case["D"], case["h"], case["w"]
    cot = vc.cotangent(case)
    inp, mgr, fwd, ref = _small_reference(case, cot)
    seen = []
    real_call = _lib.call

    def spy(name, device, *args, **kw):
        if name == "sr_mlp_volume_bwd":
            seen.append(tuple(args[1:4]))
        return real_call(name, device, *args, **kw)
    monkeypatch.setattr(_lib, "call", spy)

    R = torch.from_numpy(cot).to(DEV)
    wide = torch.zeros((B, D, h, w + 3), device=DEV)
    wide[..., :w] = R
    padded = wide[..., :w]
    assert padded.stride(2) != w * padded.stride(3)
    layouts = {"contiguous": (R, (D * h * w, h * w, 1)),
               "channels_last": (R.contiguous(memory_format=torch.channels_last), (D * h * w, 1, D)),
               "row_padded": (padded, (D * h * w, h * w, 1))}
    d_cur = {}
    for what, (g, strides) in layouts.items():
        vol, grads, _ = _run(mgr, inp, g)
        assert seen[-1] == strides, (what, seen[-1])
        _check_all(f"{case['name']}/{what}", vol, grads, fwd, ref)
        d_cur[what] = grads["d_cur_feats"]
    assert torch.equal(d_cur["contiguous"].view(torch.int32), d_cur["channels_last"].view(torch.int32))
    assert torch.equal(d_cur["contiguous"].view(torch.int32), d_cur["row_padded"].view(torch.int32))
    # vol.sum().backward(): autograd expands a scalar one
    ones = np.ones_like(cot)
    ref1 = vc.oracle_backward(case, inp, vc.mlp_dict(mgr), ones)
    vol, grads, _ = _run(mgr, inp, None)
    assert seen[-1] == (0, 0, 0), seen[-1]
    _check_all(f"{case['name']}/expanded", vol, grads, fwd, ref1)
    vol, grads_dense, _ = _run(mgr, inp, torch.ones((B, D, h, w), device=DEV))
    assert torch.equal(grads["d_cur_feats"].view(torch.int32), grads_dense["d_cur_feats"].view(torch.int32))


def test_batch_three_images_are_independent_and_d_cur_is_deterministic():
    case = vc.BATCH_CASE
    B = case["B"]
    cot = vc.cotangent(case)
    inp, mgr, fwd, ref = _small_reference(case, cot)
    R = torch.from_numpy(cot).to(DEV)
    vol, grads, _ = _run(mgr, inp, R)
    _check_all(case["name"], vol, grads, fwd, ref)
    _, again, _ = _run(mgr, inp, R)
    assert torch.equal(grads["d_cur_feats"].view(torch.int32), again["d_cur_feats"].view(torch.int32))
    _check(case["name"], "d_src_feats run to run", again["d_src_feats"], grads["d_src_feats"])
    one = {k: (v[1:2].contiguous() if v.dim() > 0 and v.shape[0] == B else v) for k, v in inp.items()}
    vol1, alone, _ = _run(mgr, one, R[1:2].contiguous())
    assert torch.equal(vol1[0].view(torch.int32), vol[1].view(torch.int32))
    assert torch.equal(alone["d_cur_feats"][0].view(torch.int32), grads["d_cur_feats"][1].view(torch.int32))
    _check(case["name"], "d_src_feats of image 1 alone vs in the batch", alone["d_src_feats"], grads["d_src_feats"][1:2])


def test_frozen_mlp_still_gives_feature_gradients():
    case = vc.FROZEN_CASE
    cot = vc.cotangent(case)
    inp, mgr, fwd, ref = _small_reference(case, cot)
    vol, grads, dmgr = _run(mgr, inp, torch.from_numpy(cot).to(DEV), frozen=True)
    _check_all(case["name"], vol, grads, fwd, ref, keys=("d_cur_feats", "d_src_feats"))
    assert all(p.grad is None and not p.requires_grad for p in dmgr.mlp.parameters())
    assert all(grads[k] is None for k in NAMES.values())
