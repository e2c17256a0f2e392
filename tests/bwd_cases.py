"""Case tables, launch-plan arithmetic and float64 references of tests/test_gpu_bwd_shapes.py: the training backward
kernels (csrc/sr_conv_bwd.hip, csrc/sr_train.hip) at the sizes training runs them at, and on ties.

Everything here runs on any device: the GPU module uses it with device="cuda:0", tests/test_bwd_cases_host.py checks the
tables themselves (plan arithmetic against the library's host-only workspace queries, the share of cotangent elements the
kink mask zeroes) on the CPU.

The plan arithmetic RESTATES the launchers (sr_wgrad_plan, sr_tr_chunk_pix, sr_bias_grad_nhwc) on purpose: a case asserts
the property it is listed for from these numbers, and the numbers are cross-checked against the library, so a plan change
makes the table fail instead of silently testing something else."""
import numpy as np
import torch
import torch.nn.functional as F

KINK_REL = 1e-4          # cotangent zeroed where |pre-activation| < KINK_REL * max|pre-activation|
KINK_SHARE_MAX = 2e-3    # ... and at most this share of the elements may be zeroed
ACT_NONE, ACT_SILU = -1.0, -2.0   # train_ops activation codes (a value >= 0 is a LeakyReLU slope, 0.0 = ReLU)


# ------------------------------------------------------------------------------------------- plan arithmetic ----
def tf_same_pads(h, w, k, s):
    def one(i):
        total = max((-(-i // s) - 1) * s + k - i, 0)
        return total // 2, total - total // 2
    (pt, pb), (pl, pr) = one(h), one(w)
    return pt, pl, pb, pr


def wgrad_plan(B, Ho, Wo, Cin, Cout):
    """sr_wgrad_plan: (co, ci) blocks of 64 x 64, items = (image, output row, 32-pixel segment), workgroups per block."""
    blocks = -(-Cout // 64) * -(-Cin // 64)
    segs = -(-Wo // 32)
    items = B * Ho * segs
    per = max(1, min(-(-512 // blocks), items))
    return dict(blocks=blocks, items=items, per=per, segs=segs)


def wgrad_workspace_bytes(plan, k):
    return plan["blocks"] * plan["per"] * k * k * 64 * 64 * 4


def colreduce_plan(npix):
    """sr_tr_chunk_pix / sr_tr_chunks: pixels per partial and number of partials of a column reduction over npix pixels."""
    chunk_pix = max(256, -(-npix // 1024))
    return dict(chunk_pix=chunk_pix, chunks=-(-npix // chunk_pix))


def bias_grad_chunks(pixels):
    """sr_bias_grad_nhwc (the atomics form, Cout % 4 != 0): grid.x, capped at 512 -- above the cap it grid-strides."""
    return max(1, min(512, -(-pixels // 256)))


# ------------------------------------------------------------------------------------------- A. convolutions ----
# prop: the structural property the row is listed for, a predicate on wgrad_plan's numbers (and the case).
# dx:   prefix of the kernel the DATA gradient runs (autograd_ops._conv_raw on the flipped weight; recorded in ops.PROFILE).
#       _conv_raw calls ops' Winograd / direct launchers without a split-K workspace (sr_conv3x3_wino_splitk_nhwc_fwd /
#       sr_conv2d_splitk_nhwc_fwd with workspace = NULL): F(2x2) Winograd (no K split) where sr_conv_prefers_wino says so and
#       the padding is symmetric, the direct implicit-GEMM kernel otherwise -- 1x1 and explicit pads included.  The F(4x4),
#       split-K and pointwise-GEMM kernels belong to ops.conv2d's dispatcher (inference) and are NOT reached from training.
def _c(name, B, ci, co, k, s, H, W, prop, dx, kind=None, bias=True, res=False, slope=None, slice_=False):
    return dict(name=name, B=B, ci=ci, co=co, k=k, s=s, H=H, W=W, kind=kind, bias=bias, res=res, slope=slope, slice=slice_,
                prop=prop, dx=dx)


CONV_CASES = [
    _c("pipe_uneven", 2, 64, 64, 3, 1, 120, 160, lambda p: p["blocks"] == 1 and p["per"] == 512 and p["items"] == 1200
       and p["items"] % p["per"] != 0, "sr_wino_kernel<", res=True, slope=0.2),
    _c("production_decoder", 8, 64, 64, 3, 1, 240, 320, lambda p: p["items"] == 19200 and p["items"] // p["per"] == 37
       and p["items"] % p["per"] != 0, "sr_wino_kernel<", slope=0.2),
    _c("deep_small", 8, 384, 256, 3, 1, 15, 20, lambda p: p["blocks"] == 24 and p["per"] == 22 and p["per"] % 4 == 2
       and p["segs"] == 1 and p["items"] > p["per"], "sr_wino_kernel<", res=True),
    _c("few_per", 1, 896, 896, 1, 1, 4, 5, lambda p: p["blocks"] == 196 and p["per"] <= 3, "sr_conv_kernel<1, 1,"),
    _c("pw_expand", 8, 256, 1536, 1, 1, 15, 20, lambda p: p["per"] == 6 and p["items"] > p["per"],
       "sr_conv_kernel<1, 1,", slope=0.2),
    _c("stride2_odd", 4, 64, 128, 3, 2, 121, 161, lambda p: p["items"] > 2 * p["per"] and p["segs"] == 3
       and p["Wo"] == 81 and p["Wo"] % 32 == 17, "sr_wino_kernel<", slope=0.2),
    _c("stride2_even", 2, 128, 256, 3, 2, 60, 80, lambda p: p["items"] > p["per"] and p["H"] % 2 == 0 and p["W"] % 2 == 0,
       "sr_wino_kernel<", bias=False, res=True),
    _c("tf_same_s2", 8, 24, 48, 3, 2, 240, 320, lambda p: p["pads"][:2] == (0, 0) and p["items"] > 2 * p["per"],
       "sr_conv_kernel<3, 1,", kind="same", bias=False),
    _c("valid_rep", 8, 64, 64, 3, 1, 120, 160, lambda p: p["pads"] == (0, 0, 0, 0) and p["items"] > 2 * p["per"],
       "sr_conv_kernel<3, 1,", kind="valid_rep"),
    _c("head", 8, 64, 1, 3, 1, 240, 320, lambda p: p["co"] % 4 != 0 and p["pixels"] == 614400
       and -(-p["pixels"] // 256) > 512 and p["items"] > 2 * p["per"], "sr_conv_kernel<3, 1,"),
    _c("rgb_in", 4, 3, 24, 3, 2, 240, 320, lambda p: p["ci"] < 4 and p["items"] > 2 * p["per"], "sr_conv_kernel<3, 1,",
       kind="same", bias=False),
    _c("slice_misaligned", 2, 48, 40, 3, 1, 64, 96, lambda p: p["ci"] % 4 == 0, "sr_wino_kernel<", slope=0.2, slice_=True),
    # (added: the row above deals one item per workgroup; the same operands with several items per workgroup)
    _c("slice_misaligned_multi", 4, 48, 40, 3, 1, 64, 96, lambda p: p["ci"] % 4 == 0 and p["items"] > p["per"],
       "sr_wino_kernel<", slope=0.2, slice_=True),
] + [
    _c(f"seg_edges_w{W}", 1, 16, 16, 3, 1, 40, W, (lambda W: lambda p: p["segs"] == -(-W // 32)
                                                   and (W % 32 in (0, 1, 31)))(W), "sr_wino_kernel<", res=True, slope=0.2)
    for W in (31, 32, 33, 64, 65)
]
CONV_BY_NAME = {c["name"]: c for c in CONV_CASES}


def conv_geometry(case):
    """pads (None = symmetric k // 2), output size, the weight gradient's plan and everything a `prop` predicate reads."""
    k, s, H, W = case["k"], case["s"], case["H"], case["W"]
    if case["kind"] == "same":
        pads, Hi, Wi = tf_same_pads(H, W, k, s), H, W
    elif case["kind"] == "valid_rep":
        pads, Hi, Wi = (0, 0, 0, 0), H + 2, W + 2      # the convolution sees the replicate-padded map
    else:
        pads, Hi, Wi = None, H, W
    pt, pl, pb, pr = pads if pads is not None else (k // 2,) * 4
    Ho, Wo = (Hi + pt + pb - k) // s + 1, (Wi + pl + pr - k) // s + 1
    p = wgrad_plan(case["B"], Ho, Wo, case["ci"], case["co"])
    p.update(pads=pads, Hi=Hi, Wi=Wi, Ho=Ho, Wo=Wo, H=H, W=W, ci=case["ci"], co=case["co"], pixels=case["B"] * Ho * Wo)
    return p


def conv_flops(case):
    g = conv_geometry(case)
    return 2.0 * g["pixels"] * case["co"] * case["ci"] * case["k"] ** 2


def conv_inputs(case, device):
    """Seeded fp32 operands: x (a channel slice [:, 2:2+C] of a wider buffer for the `slice` rows), weight, bias, residual,
    cotangent R (again a slice for those rows).  Generated on the CPU, so every device sees the same numbers."""
    g = torch.Generator().manual_seed(1000 + sum(map(ord, case["name"])))
    geo = conv_geometry(case)
    B, ci, co, k = case["B"], case["ci"], case["co"], case["k"]
    wide = 8 if case["slice"] else 0
    xw = torch.randn((B, ci + wide, case["H"], case["W"]), generator=g)
    w = torch.randn((co, ci, k, k), generator=g) / float(np.sqrt(ci * k * k))
    b = 0.1 * torch.randn((co,), generator=g) if case["bias"] else None
    r = torch.randn((B, co, geo["Ho"], geo["Wo"]), generator=g) if case["res"] else None
    Rw = torch.randn((B, co + wide, geo["Ho"], geo["Wo"]), generator=g)
    cl = lambda t: None if t is None else t.to(device).contiguous(memory_format=torch.channels_last)
    return dict(xw=cl(xw), w=w.to(device), b=None if b is None else b.to(device), res=cl(r), Rw=cl(Rw),
                sl=slice(2, 2 + ci) if wide else slice(None), sl_o=slice(2, 2 + co) if wide else slice(None))


def kink_mask(z):
    """1 where the activation's derivative at the float64 pre-activation z is unambiguous in fp32, 0 within KINK_REL of the
    kink; and the share of zeros."""
    keep = (z.detach().abs() >= KINK_REL * z.detach().abs().max()).to(z.dtype)
    return keep, float(1.0 - keep.mean())


def conv_reference(case, inp, backward=True):
    """The operator in ATen, float64, on the operands' device -> dict(y, cot, share, d_x, d_w, d_b, d_res)."""
    geo = conv_geometry(case)
    x = inp["xw"][:, inp["sl"]].double().contiguous().requires_grad_()
    w = inp["w"].double().requires_grad_()
    b = inp["b"].double().requires_grad_() if inp["b"] is not None else None
    r = inp["res"].double().requires_grad_() if inp["res"] is not None else None
    if case["kind"] == "valid_rep":
        xp = F.pad(x, (1, 1, 1, 1), mode="replicate")
    else:
        pt, pl, pb, pr = geo["pads"] if geo["pads"] is not None else (case["k"] // 2,) * 4
        xp = F.pad(x, (pl, pr, pt, pb))
    z = F.conv2d(xp, w, b, stride=case["s"])
    if r is not None:
        z = z + r
    cot = inp["Rw"][:, inp["sl_o"]].double()
    share = 0.0
    if case["slope"] is not None:
        keep, share = kink_mask(z)
        cot = cot * keep
        y = F.leaky_relu(z, case["slope"])
    else:
        y = z
    out = dict(y=y.detach(), cot=cot, share=share)
    if backward:
        (y * cot).sum().backward()
        out.update(d_x=x.grad, d_w=w.grad, d_b=None if b is None else b.grad, d_res=None if r is None else r.grad)
    return out


# ------------------------------------------------------------------------------------------- B. normalisation ---
NORM_SHAPES = {   # name: (B, C of the operand, H, W, C of the buffer it is a slice of or None)
    "c64_full": (8, 64, 240, 320, None),     # 614 400 pixels per group: chunk_pix 600 > 256, 1024 chunks
    "c24_full": (8, 24, 240, 320, None),     # C < 64: one partly filled channel block
    "c160": (8, 160, 30, 40, None),          # blockIdx.z > 0
    "c1536": (8, 1536, 15, 20, None),        # blockIdx.z up to 23
    "c30_scalar": (4, 30, 60, 80, None),     # C % 4 != 0: V = 1
    "c48_slice": (4, 48, 60, 80, 56),        # [:, 2:50] of a 56-channel buffer: C % 4 == 0, rows not 16-byte aligned: V = 1
}
NORM_MODES = [(m, a) for m in ("bn_train", "bn_eval") for a in (ACT_NONE, 0.0, ACT_SILU)] + [("in_leaky", 0.2), ("in_plain", ACT_NONE)]
NORM_DISTS = ("unit", "dc")   # x ~ N(0, 1); x = 3 + 0.1 N(0, 1)


def norm_id(shape, mode, act, dist):
    a = {ACT_NONE: "none", 0.0: "relu", ACT_SILU: "silu", 0.2: "leaky"}[act]
    return f"{shape}-{mode}-{a}-{dist}" if mode.startswith("bn") else f"{shape}-{mode}-{dist}"


NORM_CASES = [(s, m, a, d) for s in NORM_SHAPES for (m, a) in NORM_MODES for d in NORM_DISTS]
NORM_IDS = [norm_id(*c) for c in NORM_CASES]


def norm_inputs(shape_name, dist, device):
    B, C, H, W, wide = NORM_SHAPES[shape_name]
    g = torch.Generator(device=device).manual_seed(2000 + sum(map(ord, shape_name + dist)))
    cw = wide or C
    xw = torch.randn((B, H, W, cw), generator=g, device=device).permute(0, 3, 1, 2)    # channels-last storage
    if dist == "dc":
        xw = 3.0 + 0.1 * xw
    Rw = torch.randn((B, H, W, cw), generator=g, device=device).permute(0, 3, 1, 2)
    rng = np.random.default_rng(7 + C)
    mu, sd = (3.0, 0.1) if dist == "dc" else (0.0, 1.0)
    state = dict(weight=1.0 + 0.3 * rng.standard_normal(C), bias=0.2 * rng.standard_normal(C),
                 running_mean=mu + 0.3 * sd * rng.standard_normal(C), running_var=sd * sd * (0.5 + rng.random(C)))
    state = {k: torch.from_numpy(v.astype(np.float32)) for k, v in state.items()}
    sl = slice(2, 2 + C) if wide else slice(None)
    return dict(xw=xw, Rw=Rw, sl=sl, state=state, C=C)


def make_bn(inp, training, dtype, device):
    bn = torch.nn.BatchNorm2d(inp["C"], eps=1e-3)
    bn.load_state_dict({**inp["state"], "num_batches_tracked": torch.tensor(3)})
    bn.train(training)
    return bn.to(device=device, dtype=dtype)


def torch_act(z, act):
    if act == ACT_NONE:
        return z
    if act == ACT_SILU:
        return F.silu(z)
    return F.relu(z) if act == 0.0 else F.leaky_relu(z, act)


def norm_reference(mode, act, inp, backward=True):
    x = inp["xw"][:, inp["sl"]].double().contiguous().requires_grad_()
    bn = None
    if mode.startswith("bn"):
        bn = make_bn(inp, mode == "bn_train", torch.float64, x.device)
        z = bn(x)
    else:
        z = F.instance_norm(x, eps=1e-5)
    cot = inp["Rw"][:, inp["sl"]].double()
    share = 0.0
    if act >= 0.0:
        keep, share = kink_mask(z)
        cot = cot * keep
    y = torch_act(z, act)
    out = dict(y=y.detach(), cot=cot, share=share, bn=bn)
    if backward:
        (y * cot).sum().backward()
        out["d_x"] = x.grad
    return out


# ------------------------------------------------------------------------------------------- C. max-blur-pool ---
def maxblurpool_reference(x64):
    """MaxPool2d(2, stride 1) -> reflect pad (1, 2) -> blur outer([1, 3, 3, 1]) / 64 at stride 2, in ATen on x64's device."""
    C = x64.shape[1]
    m = F.max_pool2d(x64, 2, stride=1)
    a = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=x64.dtype, device=x64.device)
    filt = (a[:, None] * a[None, :] / 64.0)[None, None].repeat(C, 1, 1, 1)
    return F.conv2d(F.pad(m, (1, 2, 1, 2), mode="reflect"), filt, stride=2, groups=C)


def tie_input(kind, shape, seed):
    """fp32 maps whose 2x2 windows hold tied maxima: what a post-ReLU map looks like."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    if kind == "relu_zeros":                      # ~70 % exact zeros
        return F.relu(x - 0.5)
    if kind == "plateaus":                        # constant 3x3 plateaus (nearest-neighbour blow-up of a coarse map)
        B, C, H, W = shape
        coarse = torch.randn((B, C, -(-H // 3), -(-W // 3)), generator=g)
        return coarse.repeat_interleave(3, 2).repeat_interleave(3, 3)[:, :, :H, :W].contiguous()
    if kind == "quant3":                          # three values only
        return torch.clamp(torch.round(x), -1.0, 1.0)
    raise ValueError(kind)


def tied_window_share(x):
    """Share of the 2x2 / stride-1 windows whose maximum is attained more than once."""
    m = F.max_pool2d(x, 2, stride=1)
    n = sum((x[:, :, dy:dy + m.shape[2], dx:dx + m.shape[3]] == m).to(torch.int32) for dy in (0, 1) for dx in (0, 1))
    return float((n > 1).float().mean())


MBP_SMALL = [(h, w) for h in range(2, 7) for w in range(2, 7) if h - 1 > 2 and w - 1 > 2]   # reflect pad 2 needs H - 1 > 2
