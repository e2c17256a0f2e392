"""The training backward kernels (csrc/sr_conv_bwd.hip, csrc/sr_train.hip) at the sizes training runs them at, and on ties.

Every case compares the HIP operator (forward + backward) element-wise (parity.rel_err, range-relative) with the same
operator in ATen on float64 copies -- on the device, or on the CPU for the max-pool tie rule -- and asserts WHICH code path
it took (tests/bwd_cases.py: the weight gradient's plan, the data gradient's kernel from ops.PROFILE, the column
reductions' chunking).  Bounds are the project's operator-level ones (tests/test_gpu_conv_bwd.py,
tests/test_gpu_encoder_training.py): conv forward 1e-5, d_x / d_w / d_b 2e-5, d_residual 1e-6; normalisation forward 2e-5,
gradients 1e-4; max-blur-pool 2e-6.

Kinks: where the float64 pre-activation of a ReLU / LeakyReLU is within 1e-4 of its range of 0 the cotangent is zeroed
(both sides then see a zero upstream gradient where the derivative is ambiguous in fp32); the zeroed share is asserted
<= 2e-3.  Deterministic kernels (all but the atomics bias gradient) are run twice and compared bit for bit.

What the data gradient runs: autograd_ops._conv_raw calls ops' Winograd / direct launchers without a split-K workspace
(sr_conv3x3_wino_splitk_nhwc_fwd / sr_conv2d_splitk_nhwc_fwd with workspace = NULL), so d_x is F(2x2) Winograd
(without K split) or the direct implicit-GEMM kernel -- never F(4x4), split-K Winograd or the pointwise GEMM, which belong
to ops.conv2d's inference dispatcher.  The cases assert the kernel that really ran.

Measured errors of a run are written to $SR_BWD_PARITY_OUT (json) when that variable is set (profiles/r07_bwd_parity.json)."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import bwd_cases as bc
from parity import rel_err
from simplerecon_amd import autograd_ops, ops
from simplerecon_amd import train_ops as T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MEASURED = {}


@pytest.fixture(scope="module", autouse=True)
def _dump_measured():
    yield
    path = os.environ.get("SR_BWD_PARITY_OUT")
    if path:
        with open(path, "w") as f:
            json.dump({"metric": "parity.rel_err of the HIP operator against ATen float64 (max|a-b| / max|b|)",
                       "cases": MEASURED}, f, indent=1, sort_keys=True)


def _check(case_id, what, got, want, tol):
    e = rel_err(got, want)
    MEASURED.setdefault(case_id, {})[what] = e
    print(f"{case_id}: {what} rel err {e:.3e} (bound {tol:.0e})")
    assert torch.isfinite(got).all(), f"{case_id}: {what} has non-finite values"
    assert e <= tol, f"{case_id}: {what} rel err {e:.3e} > {tol:.1e}"


def _conv_param(t):
    return torch.nn.Parameter(t.clone())


# ------------------------------------------------------------------------------------------- A. convolutions ----
def _run_conv(case, inp, cot):
    """One forward + backward of the HIP operator -> (y, grads, names of the conv launches of the backward)."""
    geo = bc.conv_geometry(case)
    conv = torch.nn.Conv2d(case["ci"], case["co"], case["k"], stride=case["s"], padding=case["k"] // 2,
                           bias=case["bias"]).to(DEV)
    conv.weight, conv.bias = _conv_param(inp["w"]), (_conv_param(inp["b"]) if case["bias"] else None)
    xw = inp["xw"].clone(memory_format=torch.preserve_format).requires_grad_()
    x = xw[:, inp["sl"]]
    res = inp["res"].clone(memory_format=torch.preserve_format).requires_grad_() if case["res"] else None
    if case["kind"] is None:
        y = autograd_ops.conv_bias_act(x, conv, residual=res, slope=case["slope"])
    else:
        xin = T.replicate_pad(x, 1) if case["kind"] == "valid_rep" else x
        y = T.conv(xin, conv, pads=geo["pads"], residual=res, slope=case["slope"])
    ops.PROFILE = []
    try:
        y.backward(gradient=cot)
        names = [r[0] for r in ops.PROFILE]
    finally:
        ops.PROFILE = None
    torch.cuda.synchronize()
    grads = dict(d_x=xw.grad[:, inp["sl"]], d_w=conv.weight.grad, d_b=conv.bias.grad if case["bias"] else None,
                 d_res=res.grad if case["res"] else None, xw=xw.grad)
    return y.detach(), grads, names


@pytest.mark.parametrize("name", [c["name"] for c in bc.CONV_CASES])
def test_conv_bias_act_backward(name):
    """Table A of bwd_cases.CONV_CASES: weight, bias, residual and data gradient of act(conv(x) + b + residual)."""
    from simplerecon_amd import _lib
    case = bc.CONV_BY_NAME[name]
    geo = bc.conv_geometry(case)
    lib = _lib.lib()
    # the path: the weight gradient's plan (restated, cross-checked against the library) has the row's property
    if geo["pads"] is None:
        nws = lib.sr_conv_wgrad_workspace_bytes(case["B"], case["H"], case["W"], case["ci"], case["co"], case["k"], case["s"])
    else:
        nws = lib.sr_conv_wgrad_padded_workspace_bytes(case["B"], geo["Ho"], geo["Wo"], case["ci"], case["co"], case["k"])
    assert nws == bc.wgrad_workspace_bytes(geo, case["k"]) and case["prop"](geo), geo
    inp = bc.conv_inputs(case, DEV)
    ref = bc.conv_reference(case, inp)
    assert ref["share"] <= bc.KINK_SHARE_MAX, ref["share"]
    if case["slice"]:    # the cotangent arrives as a channel slice of a wider buffer too
        cw = inp["Rw"].clone(memory_format=torch.preserve_format)
        cw[:, inp["sl_o"]] = ref["cot"].float()
        cot = cw[:, inp["sl_o"]]
        assert inp["xw"][:, inp["sl"]].data_ptr() % 16 != 0 and cot.data_ptr() % 16 != 0 and not cot.is_contiguous(
            memory_format=torch.channels_last)
    else:
        cot = ref["cot"].float().contiguous(memory_format=torch.channels_last)
    y, g, names = _run_conv(case, inp, cot)
    assert len(names) == 1 and names[0].startswith(case["dx"]), (names, case["dx"])
    _check(name, "forward", y, ref["y"], 1e-5)
    _check(name, "d_x", g["d_x"], ref["d_x"], 2e-5)
    _check(name, "d_w", g["d_w"], ref["d_w"], 2e-5)
    if case["bias"]:
        _check(name, "d_b", g["d_b"], ref["d_b"], 2e-5)
    if case["res"]:
        _check(name, "d_residual", g["d_res"], ref["d_res"], 1e-6)
    if case["slice"]:    # nothing leaks into the buffer's other channels
        other = torch.ones(g["xw"].shape[1], dtype=torch.bool)
        other[inp["sl"]] = False
        assert (g["xw"][:, other] == 0).all()
    # determinism (the bias gradient of a Cout % 4 != 0 layer uses atomics: not compared)
    y2, g2, _ = _run_conv(case, inp, cot)
    assert torch.equal(y, y2) and torch.equal(g["d_x"], g2["d_x"]) and torch.equal(g["d_w"], g2["d_w"])
    if case["bias"] and case["co"] % 4 == 0:
        assert torch.equal(g["d_b"], g2["d_b"])
    if case["res"]:
        assert torch.equal(g["d_res"], g2["d_res"])


# ------------------------------------------------------------------------------------------- B. normalisation ---
def _run_norm(mode, act, inp, cot):
    xw = inp["xw"].clone(memory_format=torch.preserve_format).requires_grad_()
    x = xw[:, inp["sl"]]
    bn = None
    if mode.startswith("bn"):
        bn = bc.make_bn(inp, mode == "bn_train", torch.float32, DEV)
        y = T.batch_norm_act(x, bn, act=act)
    else:
        y = T.instance_norm_act(x, eps=1e-5, leaky=None if act == bc.ACT_NONE else act)
    y.backward(gradient=cot)
    torch.cuda.synchronize()
    return y.detach(), xw.grad[:, inp["sl"]], bn


@pytest.mark.parametrize("shape,mode,act,dist", bc.NORM_CASES, ids=bc.NORM_IDS)
def test_norm_act_backward(shape, mode, act, dist):
    """Table B: BatchNorm (training / eval statistics) and InstanceNorm with their fused activation: output, d_x, d_gamma,
    d_beta, running statistics -- at 614 400 pixels per group (pixels per chunk > 256, 1024 chunks), across several
    64-channel blocks, in the scalar (V = 1) form, on N(0, 1) and on 3 + 0.1 N(0, 1) inputs (cancellation)."""
    cid = bc.norm_id(shape, mode, act, dist)
    B, C, H, W, wide = bc.NORM_SHAPES[shape]
    plan = bc.colreduce_plan(H * W if mode.startswith("in") else B * H * W)
    if shape.endswith("_full") and mode.startswith("bn"):
        assert B * H * W > 262144 and plan["chunk_pix"] > 256 and plan["chunks"] == 1024
    inp = bc.norm_inputs(shape, dist, DEV)
    if wide or C % 4:
        assert C % 4 != 0 or inp["xw"][:, inp["sl"]].data_ptr() % 16 != 0     # the V = 1 kernels
    ref = bc.norm_reference(mode, act, inp)
    assert ref["share"] <= bc.KINK_SHARE_MAX, ref["share"]
    cot = ref["cot"].float().contiguous(memory_format=torch.channels_last)
    y, dx, bn = _run_norm(mode, act, inp, cot)
    _check(cid, "forward", y, ref["y"], 2e-5)
    _check(cid, "d_x", dx, ref["d_x"], 1e-4)
    if bn is not None:
        bnr = ref["bn"]
        _check(cid, "d_gamma", bn.weight.grad, bnr.weight.grad, 1e-4)
        _check(cid, "d_beta", bn.bias.grad, bnr.bias.grad, 1e-4)
        _check(cid, "running_mean", bn.running_mean, bnr.running_mean, 1e-5)
        _check(cid, "running_var", bn.running_var, bnr.running_var, 1e-5)
        assert int(bn.num_batches_tracked) == int(bnr.num_batches_tracked) == (4 if mode == "bn_train" else 3)
    y2, dx2, bn2 = _run_norm(mode, act, inp, cot)
    assert torch.equal(y, y2) and torch.equal(dx, dx2)
    if bn is not None:
        assert torch.equal(bn.weight.grad, bn2.weight.grad) and torch.equal(bn.bias.grad, bn2.bias.grad)
        assert torch.equal(bn.running_var, bn2.running_var)


# ------------------------------------------------------------------------------------------- C. max-blur-pool ---
def _run_mbp(x0, cot):
    """train_ops.maxblurpool forward + backward; for C % 4 != 0 -- which the forward kernel refuses, so that the operator
    never reaches sr_maxpool2_bwd_kernel, the scalar twin -- the library's backward entry point alone (y = None)."""
    x = x0.detach().to(DEV).clone(memory_format=torch.channels_last)
    g = cot.to(DEV).float().contiguous(memory_format=torch.channels_last)
    if x.shape[1] % 4 == 0:
        x.requires_grad_()
        y = T.maxblurpool(x)
        y.backward(gradient=g)
        torch.cuda.synchronize()
        return y.detach(), x.grad
    from simplerecon_amd import _lib
    lib = _lib.lib()
    b, c, h, w = x.shape
    dx = torch.full_like(x, float("nan"))
    nws = lib.sr_maxblurpool_bwd_workspace_bytes(b, h, w, c)
    ws = torch.empty((max(nws, 16),), dtype=torch.uint8, device=DEV)
    rc = lib.sr_maxblurpool_bwd_nhwc(_lib.ptr(g), *ops._strides(g), _lib.ptr(x), *ops._strides(x), _lib.ptr(dx),
                                     *ops._strides(dx), b, h, w, c, _lib.ptr(ws), nws, _lib.stream_ptr(torch.device(DEV)))
    assert rc == 0
    torch.cuda.synchronize()
    return None, dx


def _mbp_compare(cid, x0, ref_device="cpu"):
    xr = x0.to(ref_device).double().requires_grad_()
    yr = bc.maxblurpool_reference(xr)
    cot = torch.randn(tuple(yr.shape), generator=torch.Generator().manual_seed(6)).to(ref_device)
    (yr * cot.double()).sum().backward()
    y, dx = _run_mbp(x0, cot)
    if y is not None:
        _check(cid, "forward", y, yr.detach(), 2e-6)
    _check(cid, "d_x", dx, xr.grad, 2e-6)
    y2, dx2 = _run_mbp(x0, cot)
    assert (y is None or torch.equal(y, y2)) and torch.equal(dx, dx2)


@pytest.mark.parametrize("C", [6, 64], ids=["scalar", "vec4"])
@pytest.mark.parametrize("kind", ["relu_zeros", "plateaus", "quant3"])
def test_maxblurpool_backward_on_ties(kind, C):
    """The gradient of a tied 2x2 window goes to its FIRST maximum in row-major order (ATen's rule, reference: ATen on the
    CPU): post-ReLU maps are full of exact-zero ties."""
    x0 = bc.tie_input(kind, (2, C, 37, 50), seed=5)
    assert bc.tied_window_share(x0) > 0.10
    _mbp_compare(f"maxblurpool-{kind}-C{C}", x0)


@pytest.mark.parametrize("C", [6, 64], ids=["scalar", "vec4"])
def test_maxblurpool_backward_inf_and_nan(C):
    """One +inf and one NaN element: NaN wins a window (like ATen); the output's non-finite positions and the finite rest
    agree, the gradient (finite: it only routes the cotangent) agrees everywhere.  (The forward kernel used fmaxf, which
    drops a NaN operand: the NaN vanished from the output while the backward routed the gradient to it.)"""
    x0 = torch.randn((2, C, 21, 30), generator=torch.Generator().manual_seed(8))
    x0[0, 1, 7, 9] = float("inf")
    x0[1, C - 1, 12, 20] = float("nan")
    xr = x0.double().requires_grad_()
    yr = bc.maxblurpool_reference(xr)
    cot = torch.randn(tuple(yr.shape), generator=torch.Generator().manual_seed(6))
    (yr * cot.double()).sum().backward()
    y, dx = _run_mbp(x0, cot)
    yr = yr.detach()
    assert torch.isnan(yr).any() and torch.isinf(yr).any()
    if y is not None:
        yc = y.cpu()
        assert torch.equal(torch.isnan(yc), torch.isnan(yr)) and torch.equal(torch.isinf(yc), torch.isinf(yr))
        fin = torch.isfinite(yr)
        assert rel_err(yc[fin], yr[fin]) < 2e-6
    assert torch.isfinite(xr.grad).all()
    _check(f"maxblurpool-nonfinite-C{C}", "d_x", dx, xr.grad, 2e-6)


@pytest.mark.parametrize("C", [6, 64], ids=["scalar", "vec4"])
@pytest.mark.parametrize("hw", bc.MBP_SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_maxblurpool_backward_smallest_maps(hw, C):
    """Every map of up to 6 x 6 that the reflect pad accepts: the reflections of sr_blurpool_bwd_kernel that coincide
    (y == 1 and y == Hm - 2 at once for Hm = 3, y == 1 and y == Hm - 3 for Hm = 4)."""
    x0 = bc.tie_input("relu_zeros", (3, C, hw[0], hw[1]), seed=11 + hw[0] * 7 + hw[1])
    _mbp_compare(f"maxblurpool-{hw[0]}x{hw[1]}-C{C}", x0)


def test_maxblurpool_backward_full_size():
    """(8, 64, 240, 320): the grid-stride loops (39 M elements on at most 8192 workgroups); reference on the device."""
    x0 = torch.randn((8, 240, 320, 64), generator=torch.Generator(device=DEV).manual_seed(9), device=DEV).permute(0, 3, 1, 2)
    assert x0.numel() // 4 > 8192 * 256
    _mbp_compare("maxblurpool-full", x0, ref_device=DEV)


# ------------------------------------------------------------------------------------------- D. the rest --------
def _run_dw_se(x0, mods, pads, cot):
    dw, r, e = mods
    for m in mods:
        m.zero_grad()
    x = x0.clone(memory_format=torch.preserve_format).requires_grad_()
    y = T.squeeze_excite(T.dwconv3x3(x, dw, pads), r, e)
    y.backward(gradient=cot)
    torch.cuda.synchronize()
    return y.detach(), x.grad, [p.grad.clone() for m in mods for p in m.parameters()]


@pytest.mark.parametrize("cfg", [(8, 640, 30, 40, 1), (8, 960, 30, 40, 2)], ids=["c640_s1", "c960_s2_same"])
def test_depthwise_and_squeeze_excite_at_size(cfg):
    """dwconv3x3 (TF-SAME) + squeeze_excite on the image-prior encoder's largest depthwise maps: many chunks in
    sr_dw_wgrad_kernel, sr_rowsum_nhwc and the MODE 3 column reduction."""
    B, Cn, H, W, s = cfg
    cid = f"dw_se-c{Cn}-s{s}"
    rd = Cn // 16
    torch.manual_seed(Cn)
    dw = torch.nn.Conv2d(Cn, Cn, 3, stride=s, padding=1, groups=Cn, bias=False)
    r, e = torch.nn.Conv2d(Cn, rd, 1), torch.nn.Conv2d(rd, Cn, 1)
    mods = [m.to(DEV) for m in (dw, r, e)]
    x0 = torch.randn((B, H, W, Cn), generator=torch.Generator(device=DEV).manual_seed(10), device=DEV).permute(0, 3, 1, 2)
    pads = bc.tf_same_pads(H, W, 3, s)
    assert bc.colreduce_plan(H * W)["chunks"] >= 4 and (s == 1 or pads[:2] == (0, 0))
    xr = x0.double().requires_grad_()
    wr = [p.detach().double().requires_grad_() for m in mods for p in m.parameters()]
    d = F.conv2d(F.pad(xr, (pads[1], pads[3], pads[0], pads[2])), wr[0], stride=s, groups=Cn)
    gate = torch.sigmoid(F.conv2d(F.silu(F.conv2d(d.mean((2, 3), keepdim=True), wr[1], wr[2])), wr[3], wr[4]))
    yr = d * gate
    cot = torch.randn(tuple(yr.shape[i] for i in (0, 2, 3, 1)), generator=torch.Generator(device=DEV).manual_seed(11),
                      device=DEV).permute(0, 3, 1, 2)
    (yr * cot.double()).sum().backward()
    y, dx, dps = _run_dw_se(x0, mods, pads, cot)
    _check(cid, "forward", y, yr.detach(), 2e-5)
    _check(cid, "d_x", dx, xr.grad, 1e-4)
    for nm, got, want in zip(("d_dw", "d_w1", "d_b1", "d_w2", "d_b2"), dps, wr):
        _check(cid, nm, got, want.grad, 1e-4)
    y2, dx2, dps2 = _run_dw_se(x0, mods, pads, cot)
    assert torch.equal(y, y2) and torch.equal(dx, dx2) and all(torch.equal(a, b) for a, b in zip(dps, dps2))


@pytest.mark.parametrize("shape", [(8, 64, 120, 160), (3, 12, 37, 53)], ids=["c64_120x160", "odd_37x53"])
def test_upsample2x_backward_at_size(shape):
    B, Cn, H, W = shape
    x0 = torch.randn((B, H, W, Cn), generator=torch.Generator(device=DEV).manual_seed(12), device=DEV).permute(0, 3, 1, 2)
    cot = torch.randn((B, 2 * H, 2 * W, Cn), generator=torch.Generator(device=DEV).manual_seed(13), device=DEV).permute(0, 3, 1, 2)
    xr = x0.double().requires_grad_()
    F.interpolate(xr, scale_factor=2, mode="bilinear", align_corners=False).backward(gradient=cot.double())
    outs = []
    for _ in range(2):
        x = x0.clone(memory_format=torch.preserve_format).requires_grad_()
        autograd_ops.upsample2x(x).backward(gradient=cot)
        outs.append(x.grad)
    _check(f"upsample2x-{B}x{Cn}x{H}x{W}", "d_x", outs[0], xr.grad, 1e-6)
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("act", [bc.ACT_NONE, 0.0, 0.2, bc.ACT_SILU], ids=["none", "relu", "leaky", "silu"])
def test_add_act_backward_at_size(act):
    """The residual join at 39 M elements.  ReLU / LeakyReLU gradients select or scale the cotangent (1e-6, the existing
    residual-join bound); SiLU' is evaluated in fp32 with the fast exponential: the operator-level gradient bound 2e-5."""
    shape = (8, 240, 320, 64)
    a0, b0, R = (torch.randn(shape, generator=torch.Generator(device=DEV).manual_seed(20 + i), device=DEV).permute(0, 3, 1, 2)
                 for i in range(3))
    ar, br = a0.double().requires_grad_(), b0.double().requires_grad_()
    z = ar + br
    cot = R.double()
    if act >= 0.0:
        keep, share = bc.kink_mask(z)
        assert share <= bc.KINK_SHARE_MAX, share
        cot = cot * keep
    yr = bc.torch_act(z, act)
    (yr * cot).sum().backward()
    outs = []
    for _ in range(2):
        a, b = a0.clone(memory_format=torch.preserve_format).requires_grad_(), b0.clone(memory_format=torch.preserve_format).requires_grad_()
        y = T.add(a, b, act=act)
        y.backward(gradient=cot.float())
        outs.append((y.detach(), a.grad, b.grad))
    cid = f"add-{act}"
    _check(cid, "forward", outs[0][0], yr.detach(), 2e-5)
    tol = 2e-5 if act == bc.ACT_SILU else 1e-6
    _check(cid, "d_a", outs[0][1], ar.grad, tol)
    _check(cid, "d_b", outs[0][2], br.grad, tol)
    assert all(torch.equal(p, q) for p, q in zip(outs[0], outs[1]))


def test_stem7x7_weight_gradient_full_size():
    """(8, 3, 480, 640): the stem's weight gradient = a 1x1 weight gradient over the unfolded image, 5 images per chunk
    (256 MB of columns), 76 800 pixels per image -- 24 000 items on 512 workgroups, partials of the chunks added in order."""
    torch.manual_seed(7)
    conv = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False).to(DEV)
    x0 = torch.randn((8, 3, 480, 640), generator=torch.Generator(device=DEV).manual_seed(30), device=DEV)
    cot = torch.randn((8, 240, 320, 64), generator=torch.Generator(device=DEV).manual_seed(31), device=DEV).permute(0, 3, 1, 2)
    per = max(1, min(8, (1 << 28) // (240 * 320 * 160 * 4)))
    assert 1 < per < 8      # several chunks, the last one shorter
    wr = conv.weight.detach().double().requires_grad_()
    F.conv2d(x0.double(), wr, stride=2, padding=3).backward(gradient=cot.double())
    outs = []
    for _ in range(2):
        conv.zero_grad()
        y = T.stem7x7(x0, conv)
        y.backward(gradient=cot)
        outs.append(conv.weight.grad.clone())
    _check("stem7x7-full", "d_w", outs[0], wr.grad, 1e-4)
    assert torch.equal(outs[0], outs[1])
