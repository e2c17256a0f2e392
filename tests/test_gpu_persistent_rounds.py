"""The persistent inference kernels past each workgroup's first work item (tests/persistent_cases.py): sr_t16_kernel,
sr_stem_kernel, sr_conv1x1_stats_kernel (csrc/sr_matching.hip) and the three F(4x4) Winograd forms (csrc/sr_wino4.hip) at batch
sizes, chosen from the device's CU count, at which every workgroup takes a second item and part of them a third -- the LDS
buffers handed over between items, the prefetch registers that hold the next item's data, the barrier protocols and the XCD
index remaps are what a later item runs and a first item does not.

Every case runs the operator through its existing entry point and compares EVERY output element with the same operator in
ATen float64 on the device, at the bounds the project already holds these kernels to (parity.rel_err: max|a - b| / max|b|):
t16 1e-5, stem 1e-5 (the bound of an fp32-MFMA conv forward), conv1x1_stats 1e-5 (output, mean) / 2e-5 (rstd), F(4x4) 2e-5
plus bit-equality of its three forms.  A failure names the worst element's work item and, from the restated launch plan, the
workgroup and the trip that computed it.

The measured error per trip (max over the items that were some workgroup's trip 0, 1, ...) is written to
$SR_PERSISTENT_PARITY_OUT (json) when that variable is set (profiles/persistent_rounds_parity.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import persistent_cases as pc
from parity import rel_err
from simplerecon_amd import _lib, ops, synthetic
from test_gpu_wino4 import _ref64, _run

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_measured():
    yield
    path = os.environ.get("SR_PERSISTENT_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"metric": "parity.rel_err of the HIP operator against ATen float64 (max|a-b| / max|b|), maximum over the "
                                 "work items of each trip (trip 0 = a workgroup's first item)",
                       "compute_units": _cus(), "cases": MEASURED}, f, indent=1, sort_keys=True)


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _batch(case):
    B = pc.shape_for(case, _cus())
    if B is None:
        pytest.skip(f"{case['name']}: no batch size has the case's property on {_cus()} compute units")
    assert pc.has_property(case, B, _cus())
    return B


def _randn(shape, seed, nhwc=True):
    g = torch.Generator(device=DEV).manual_seed(seed)
    if not nhwc:
        return torch.randn(shape, generator=g, device=DEV)
    b, c, h, w = shape
    return torch.randn((b, h, w, c), generator=g, device=DEV).permute(0, 3, 1, 2)    # channels-last storage


def _nan_out(b, c, h, w):
    """An output buffer that holds no answer: the caching allocator may hand a launch the block a previous, identical launch
    wrote, and an item that was never written would then look right."""
    return ops.empty_nhwc(b, c, h, w, DEV).fill_(float("nan"))


def _where(case, B, plan, item):
    w_of, t_of = pc.attribution(plan)
    unit = "workgroup" if plan["workers"] == plan["grid"] else "4-wave group"
    return f"work item {item} of {plan['total']} = trip {int(t_of[item])} of {unit} {int(w_of[item])} (of {plan['workers']})"


def _check(case, B, got, ref, bound, what="output", form=None):
    """Every element of `got` against `ref` (float64), attributed to work items and trips; records and asserts."""
    plan = pc.case_plan(case, B, _cus(), form)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = (got.double() - ref).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))    # (a value that is not finite: an item never written)
    scale = max(float(ref.abs().max()), 1e-30)
    idx = [torch.arange(n, device=err.device).view([-1 if d == i else 1 for d in range(4)]) for i, n in enumerate(err.shape)]
    item = pc.item_of_output(case, B, *idx).expand(err.shape).reshape(-1)
    per_item = torch.zeros(plan["total"], dtype=torch.float64, device=err.device)
    per_item.scatter_reduce_(0, item, err.reshape(-1), "amax", include_self=True)
    per_item = per_item.cpu().numpy() / scale
    w_of, t_of = pc.attribution(plan)
    trips = np.zeros(int(t_of.max()) + 1)
    np.maximum.at(trips, t_of, per_item)
    worst = int(per_item.argmax())
    if np.isfinite(per_item[worst]):
        assert abs(per_item[worst] - rel_err(got, ref)) <= 1e-12 * max(per_item[worst], 1e-30)    # the metric is parity.rel_err
    MEASURED.setdefault(case["name"], {"batch": B, "items": plan["total"], "workgroups": plan["grid"]})[what] = {
        "bound": bound, "per_trip": [float(f"{e:.3e}") for e in trips], "items_per_trip": np.bincount(t_of).tolist()}
    print(f"{case['name']} {what}: B {B}, {plan['total']} items on {plan['grid']} workgroups, rel err per trip "
          + " ".join(f"{e:.2e}" for e in trips))
    assert per_item[worst] <= bound, (f"{case['name']} {what}: rel err {per_item[worst]:.3e} > {bound:.1e} at "
                                      f"{_where(case, B, plan, worst)}; per trip {[f'{e:.2e}' for e in trips]}")
    return trips


def _assert_same(case, B, got, want, form, what):
    """Bit-equality of two launches, naming the first element that differs by item, worker and trip of `form`'s plan."""
    if torch.equal(got, want):
        return
    bad = (got != want) | torch.isnan(got)
    b, c, y, x = (int(v) for v in bad.nonzero()[0])
    item = int(pc.item_of_output(case, B, b, c, y, x))
    plan = pc.case_plan(case, B, _cus(), form)
    raise AssertionError(f"{case['name']}: {what}: {int(bad.sum())} elements differ, the first at (b {b}, c {c}, y {y}, x {x}) in "
                         f"{_where(case, B, plan, item)}")


# ------------------------------------------------------------------------------------------- conv3x3, <= 16 channels ----
def _t16_into(x, conv, stats, in_leaky, out):
    """sr_conv3x3_c16_nhwc_fwd into a given channels-last view (ops.conv3x3_c16 allocates its output)."""
    b, ci, h, w = x.shape
    wp, bias = ops._pack_c16(conv)
    isb, isp = ops._strides(x)
    osb, osp = ops._strides(out)
    with _lib.on_device(x.device):
        rc = _lib.lib().sr_conv3x3_c16_nhwc_fwd(_lib.ptr(x), isb, isp, _lib.ptr(stats),
                                                C.c_float(-1.0 if in_leaky is None else in_leaky), _lib.ptr(wp), _lib.ptr(bias),
                                                _lib.ptr(out), osb, osp, b, h, w, ci, conv.out_channels,
                                                int(conv.padding_mode == "replicate"), C.c_float(-1.0),
                                                _lib.stream_ptr(x.device))
    _lib.check(rc, "sr_conv3x3_c16_nhwc_fwd")


T16 = [c for c in pc.CASES if c["op"] == "t16"]


@pytest.mark.parametrize("case", T16, ids=[c["name"] for c in T16])
def test_t16_later_items(case):
    """conv3x3(act(InstanceNorm(x))) with 5 x 5 ragged items per image over 2 1/3 rounds of 3 workgroups per CU: the barrier that
    protects LDS buffer 0 from the previous item, two rounds under the XCD remap and the tail in launch order; all four
    <NORM, IN_ACT> instances; one case reads from and writes into channel slices of wider buffers."""
    B = _batch(case)
    ci, co, H, W = case["ci"], case["co"], case["H"], case["W"]
    conv = synthetic.seeded_fill_(nn.Conv2d(ci, co, 3, padding=1, padding_mode=case["mode"]), seed=ci + co).to(DEV)
    in_leaky = 0.2 if case["act"] else None
    guard = 4 if case["sliced"] else 0
    buf = _randn((B, ci + 2 * guard, H, W), 11 + ci) * 1.7 + 0.4
    if guard:
        buf[:, :guard] = float("nan")
        buf[:, guard + ci:] = float("nan")
    x = buf[:, guard:guard + ci] if guard else buf
    with torch.inference_mode():
        stats = ops.instance_norm_stats(x) if case["norm"] else None
        if guard:
            wide = ops.empty_nhwc(B, co + 2 * guard, H, W, DEV).fill_(7.0)
            y = wide[:, guard:guard + co]
            _t16_into(x, conv, stats, in_leaky, y)
            dense = ops.conv3x3_c16(x.contiguous(memory_format=torch.channels_last), conv, in_stats=stats, in_leaky=in_leaky)
        else:
            y = ops.conv3x3_c16(x, conv, in_stats=stats, in_leaky=in_leaky)
        xd = x.double()
        if case["norm"]:
            xd = F.instance_norm(xd, eps=1e-5)
        if case["act"]:
            xd = F.leaky_relu(xd, 0.2)
        xd = F.pad(xd, (1, 1, 1, 1), mode="replicate" if case["mode"] == "replicate" else "constant")
        ref = F.conv2d(xd, conv.weight.double(), conv.bias.double())
    torch.cuda.synchronize()
    trips = _check(case, B, y, ref, 1e-5)
    assert len(trips) >= 3
    if guard:
        _assert_same(case, B, y, dense, None, "the launch on channel slices against the one on dense tensors")
        assert bool((wide[:, :guard] == 7).all()) and bool((wide[:, guard + co:] == 7).all()), "guard channels written"


# ------------------------------------------------------------------------------------------- stem 7x7 / stride 2 --------
STEM = [c for c in pc.CASES if c["op"] == "stem"]


@pytest.mark.parametrize("case", STEM, ids=[c["name"] for c in STEM])
def test_stem_later_items(case):
    """4 x 5 ragged 16 x 16 tiles per image over 2 1/3 rounds of 2 workgroups per CU: the next tile's patch is fetched into
    registers under the MFMA loop and stashed into the single LDS patch buffer between two barriers."""
    B = _batch(case)
    H, W = case["H"], case["W"]
    conv = synthetic.seeded_fill_(nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=not case["bn"]), seed=3).to(DEV)
    bn = synthetic.seeded_fill_(nn.BatchNorm2d(64), seed=5).to(DEV).eval() if case["bn"] else None
    x = _randn((B, 3, H, W), 17, nhwc=False)
    with torch.inference_mode():
        ho, wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
        y = ops.stem7x7(x, conv, bn, leaky=case["leaky"], out=_nan_out(B, 64, ho, wo))
        y_cl = ops.stem7x7(x.contiguous(memory_format=torch.channels_last), conv, bn, leaky=case["leaky"],
                           out=_nan_out(B, 64, ho, wo))
        ref = F.conv2d(x.double(), conv.weight.double(), None if conv.bias is None else conv.bias.double(), stride=2, padding=3)
        if bn is not None:
            ref = F.batch_norm(ref, bn.running_mean.double(), bn.running_var.double(), bn.weight.double(), bn.bias.double(),
                               False, 0.0, bn.eps)
        if case["leaky"] is not None:
            ref = F.leaky_relu(ref, case["leaky"])
    torch.cuda.synchronize()
    trips = _check(case, B, y, ref, 1e-5)
    assert len(trips) >= 3
    _assert_same(case, B, y_cl, y, None, "a channels-last image against the NCHW image")


# ------------------------------------------------------------------------------------------- conv1x1 + statistics -------
def test_conv1x1_stats_later_items():
    """Conv2d(64, 128, 1) + InstanceNorm statistics on 17 x 23 maps (7 items per image, the last one 7 pixels) over 2 1/3 rounds of
    3 workgroups per CU: the next item's pixels wait in registers across the item, xs / ys / red are reused item after item."""
    case = pc.BY_NAME["c1s_64_128"]
    B = _batch(case)
    H, W = case["H"], case["W"]
    conv = synthetic.seeded_fill_(nn.Conv2d(64, 128, 1), seed=6).to(DEV)
    x = _randn((B, 64, H, W), 23) * 1.3 + 0.2
    with torch.inference_mode():
        y, stats = ops.conv1x1_stats(x, conv, eps=1e-5)
        y2, stats2 = ops.conv1x1_stats(x, conv, eps=1e-5)
        ref = F.conv2d(x.double(), conv.weight.double(), conv.bias.double())
        mean = ref.mean(dim=(2, 3))
        rstd = 1.0 / torch.sqrt(ref.var(dim=(2, 3), unbiased=False) + 1e-5)
    torch.cuda.synchronize()
    trips = _check(case, B, y, ref, 1e-5)
    assert len(trips) >= 3
    plan = pc.case_plan(case, B, _cus())
    w_of, t_of = pc.attribution(plan)
    for what, got, want, bound in (("mean", stats[:, 0], mean, 1e-5), ("rstd", stats[:, 1], rstd, 2e-5)):
        assert bool(torch.isfinite(got).all())
        per_image = ((got.double() - want).abs().amax(dim=1) / want.abs().max()).cpu().numpy()
        b = int(per_image.argmax())
        MEASURED[case["name"]][what] = {"bound": bound, "worst": float(f"{per_image[b]:.3e}")}
        print(f"{case['name']} {what}: rel err {per_image[b]:.2e}")
        items = range(7 * b, 7 * b + 7)
        assert per_image[b] <= bound, (f"fused {what}: rel err {per_image[b]:.3e} > {bound:.1e} in image {b}, whose items "
                                       f"{items[0]}..{items[-1]} are trips {[int(t_of[i]) for i in items]} of workgroups "
                                       f"{[int(w_of[i]) for i in items]}")
    _assert_same(case, B, y2, y, None, "a second launch against the first")
    assert torch.equal(stats, stats2), "the statistics of two launches differ"


# ------------------------------------------------------------------------------------------- F(4x4) Winograd ------------
def _w4_case(case, min_trips):
    B = _batch(case)
    ci, co, H, W = case["ci"], case["co"], case["H"], case["W"]
    torch.manual_seed(ci * 131 + co + H)
    conv = nn.Conv2d(ci, co, 3, padding=1).to(DEV)
    x = _randn((B, ci, H, W), 31 + ci + 7 * H).contiguous(memory_format=torch.channels_last)
    res = _randn((B, co, H, W), 37 + co + 7 * H).contiguous(memory_format=torch.channels_last)
    with torch.inference_mode():
        y_ws = _run("w4_ws", x, conv, res, 0.2, out=_nan_out(B, co, H, W))
        torch.cuda.synchronize()     # (a protocol error of this form shows here, before anything else is queued)
        ref = _ref64(x, conv, res, 0.2)
        trips = _check(case, B, y_ws, ref, 2e-5, what="w4_ws")
        assert len(trips) >= min_trips
        for form in ("w4", "w4_pp"):
            y = _run(form, x, conv, res, 0.2, out=_nan_out(B, co, H, W))
            torch.cuda.synchronize()
            _assert_same(case, B, y, y_ws, form, f"form {form} against the wave-specialised form")
            MEASURED[case["name"]][form] = {"equal_to_w4_ws": True,
                                            "trips": int(pc.case_plan(case, B, _cus(), form)["trip"].max()) + 1}
            del y


def test_wino4_one_slab_protocol_over_several_items():
    """Cin = 16 is one slab per item (S = 1): sr_wino4ws_kernel then closes an item on EVERY tick, adds barrier B4 and moves the
    residual loads behind the cursor advance.  Both roles must execute the same number of __syncthreads(); counted on the source
    for a workgroup that walks n items (K = n S ticks):
      T waves: 1 (raw[0] visible) + one F per tick k = 0 .. K (K + 1) + B2, B3 for every item that closed before the last tick
               (2 (n - 1)) + with S = 1 one B4 for each of those (n - 1) + B2, B3 after the loop (2);
      M waves: 2 (raw[0] visible, F of tick 0) + one F per tick k = 1 .. K (K) + B2, B3 per item (2 n) + with S = 1 one B4 for
               every item but the first (n - 1).
      S = 1:  n = 1: 5 = 5;  n = 2: 9 = 9;  n = 3: 13 = 13  (4 n + 1 for both roles);
      S >= 2: K + 2 n + 2 for both (S = 2: 6, 10, 14 for n = 1, 2, 3),
    and in the same order: ... F(k - 1) | B2 B3 B4 F(k) | ... on the T side against ... F(k - 1) B2 B3 | B4 F(k) B2 B3 | ... on the
    M side.  The case runs 60 x 56 x 72 on 256 CUs: 1200 items, every workgroup takes four or five."""
    _w4_case(pc.BY_NAME["w4_s1_16_64"], 3)


W4_MULTI = [c for c in pc.CASES if c["op"] == "w4" and c["kind"] == "multi" and c["name"] != "w4_s1_16_64"]


@pytest.mark.parametrize("case", W4_MULTI, ids=[c["name"] for c in W4_MULTI])
def test_wino4_later_items(case):
    """4 x 5 ragged regions per image, residual + LeakyReLU(0.2), over 2 1/3 rounds of the 4-wave form's grid (4 2/3 of the
    wave-specialised form's) at slab counts 3, 2 (with a Cin tail), 8 (two output-channel blocks; at 40 x 72 a walk crosses from block 0 into block 1, which the
    40 items per image of 56 x 72 never let happen) and 12."""
    _w4_case(case, 3)


W4_UNEVEN = [c for c in pc.CASES if c["op"] == "w4" and c["kind"] != "multi"]


@pytest.mark.parametrize("case", W4_UNEVEN, ids=[c["name"] for c in W4_UNEVEN])
def test_wino4_one_round_with_an_uneven_total(case):
    """One round whose total is no multiple of 8: the XCD split hands one workgroup two items and lets others return with none."""
    _w4_case(case, 2)
