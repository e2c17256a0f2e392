"""Per-kernel guard bands: every operand of an op sits inside a larger allocation full of NaN (hostile_memory.guarded), every
`out=` destination is such a view, and the result must not notice.

Each case
  1. runs the op on plain dense operands,
  2. runs it again on guarded operands (and into a guarded destination), with the workspaces dropped and `torch.empty`
     poisoned, so that scratch and wrapper-allocated outputs start as NaN too,
  3. asserts through ops.PROFILE that both runs launched the same kernel symbols (the conv family and the matching encoder's
     profiled kernels leave records; the other ops pick their instantiation inside the library from the alignment of
     pointers and strides, which the guarded views share with dense tensors),
  4. asserts that the guarded result is finite and bit-equal to the plain one,
  5. asserts that every guard element and every input is bitwise unchanged.
The misaligned variant (offset=1: base address one element off a 16-byte boundary) may legitimately run another kernel;
its result is then compared with a float64 reference at the tolerance of the op's own parity test.  A wrapper that refuses
such a view must do so loudly: the refusal is asserted.

Layout of the guarded operands, per case list:
  * "image": lead / tail channels in each pixel stride, a gap between images, two pixel rows at both ends;
  * "image, batch-dense": the same without the gap -- the LDS-tiled pointwise GEMM only serves batch-dense maps, with a gap
    the dispatcher would (rightly) pick the other kernel;
  * "ends": the tensor keeps its dense layout between two guard bands -- wrappers that take no strided view (gates, pooled
    sums, statistics, NCHW images)."""
import contextlib
import ctypes as C

import pytest
import torch
import torch.nn.functional as F
from torch import nn

from hostile_memory import assert_unaffected, guarded, poisoned_empty
from parity import TOL, rel_err
from simplerecon_amd import _lib, ops, synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def _rand(shape, seed, nhwc=True):
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(shape, generator=g).to(DEV)
    return t.contiguous(memory_format=torch.channels_last) if nhwc and len(shape) == 4 else t


def _profiled(fn):
    prof = []
    ops.PROFILE = prof
    try:
        out = fn()
    finally:
        ops.PROFILE = None
    return out, [r[0] for r in prof]


def _tuple(x):
    return tuple(x) if isinstance(x, (tuple, list)) else (x,)


def run_case(op, tensors, *, out_shape=None, out_dtype=torch.float32, inout=(), ends_only=(), offset=0, guard_kw=None,
             reference=None, tol=None, refuses=None, grad=False, loose=(), what=""):
    """`op(t, out)`: t maps operand names to tensors (None stays None), out is None or the destination view.  `inout`:
    operands the op updates in place (not checked for being unchanged; the plain run gets its own copies).  `ends_only`:
    operands guarded in their dense layout.  `refuses` = (exception type, message pattern) for a view the wrapper must reject.
    `grad`: the op runs a backward pass (no inference mode).  `loose`: indices of outputs that are summed with atomics --
    not bit-reproducible run to run, so compared range-relative at parity.TOL, the bound their own tests hold them to run to
    run and against the oracle; every other output must be bit-equal."""
    guard_kw = dict(guard_kw or {})
    with (contextlib.nullcontext() if grad else torch.inference_mode()):
        fresh = {k: (v.clone(memory_format=torch.preserve_format) if k in inout else v) for k, v in tensors.items()}
        plain, names = _profiled(lambda: op(fresh, None))
        plain = tuple(p.clone() if p is not None else None for p in _tuple(plain))
        torch.cuda.synchronize()
        pairs = {k: guarded(v, offset=offset, **({"dense": True} if k in ends_only or v.dim() != 4 else guard_kw))
                 for k, v in tensors.items() if v is not None}
        views = {k: (pairs[k][1] if v is not None else None) for k, v in tensors.items()}
        dest = guarded(torch.full(out_shape, NAN, dtype=out_dtype, device=DEV), offset=offset, **guard_kw) \
            if out_shape is not None else None
        ops._WORKSPACES.clear()
        if refuses is not None:
            with pytest.raises(refuses[0], match=refuses[1]):
                op(views, None if dest is None else dest[1])
            return
        with poisoned_empty(0xFF):
            got, gnames = _profiled(lambda: op(views, None if dest is None else dest[1]))
        got = _tuple(got)
        torch.cuda.synchronize()
    ops._WORKSPACES.clear()   # (scratch that was allocated poisoned is not kept for other tests)
    guards = list(pairs.values()) + ([dest] if dest is not None else [])
    inputs = [(views[k], tensors[k]) for k in pairs if k not in inout]
    print(f"{what}: kernels {names} / guarded {gnames}")

    def exact():
        ok = [i for i in range(len(plain)) if i not in loose]
        assert_unaffected([plain[i] for i in ok], [got[i] for i in ok], guards, inputs, what=what)
        for i in loose:
            err = rel_err(got[i], plain[i])
            print(f"{what}: output {i} (atomics) differs from the dense run by {err:.2e} of its range (bound {TOL:.0e})")
            assert bool(torch.isfinite(got[i]).all()) and err <= TOL, (what, i, err)
    if offset == 0:
        assert gnames == names, f"{what}: guarded operands ran {gnames}, dense ones {names}"
        return exact()
    if names and gnames == names:   # the misaligned view was served by the very same kernel symbols
        return exact()
    if not names and reference is None:   # (an op without PROFILE records and without a scalar path of its own)
        return exact()
    # the misaligned variant took (or, for an op that leaves no PROFILE record, may have taken) another kernel: the same
    # operator in another instantiation, compared with the float64 reference
    assert reference is not None and tol is not None, f"{what}: {gnames} != {names} and no reference to compare with"
    refs = _tuple(reference(tensors))
    for g, r in zip(got, refs):
        err = rel_err(g, r)
        print(f"{what}: misaligned variant vs float64 reference: {err:.2e} (bound {tol:.0e})")
        assert bool(torch.isfinite(g).all()) and err < tol, (what, err)
    assert_unaffected((), (), guards, inputs, what=what)


# ============================================================ ops.conv2d ===================================================

def _conv_ref(conv, stride=1, bn=None, act=0.2, tf_same=False):
    def ref(t):
        x = t["x"].double()
        if t.get("gate") is not None:
            x = x * t["gate"].double()[:, :, None, None]
        k = conv.kernel_size[0]
        w, b = conv.weight.double(), conv.bias.double() if conv.bias is not None else None
        if tf_same:
            pt, pl, pb, pr = ops.tf_same_pads(x.shape[2], x.shape[3], k, stride)
            y = F.conv2d(F.pad(x, (pl, pr, pt, pb)), w, b, stride=stride)
        elif conv.padding_mode == "replicate":
            y = F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), w, b, stride=stride)
        else:
            y = F.conv2d(x, w, b, stride=stride, padding=k // 2)
        if bn is not None:
            scale, shift = ops.bn_affine(bn)
            y = y * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
        if t.get("res") is not None:
            y = y + t["res"].double()
        return F.silu(y) if act == "silu" else F.leaky_relu(y, act) if act is not None else y
    return ref


def _conv_case(shape, *, k=3, stride=1, padding_mode="zeros", tf_same=False, act=0.2, gate=False, offset=0, guard_kw=None,
               expect=None, refuses=None, what=""):
    """conv2d with bias, residual and an activation (LeakyReLU(0.2), or SiLU where the route's own test uses it) into a guarded
    destination; `expect`: a prefix the first kernel symbol must have (the route the case is about)."""
    b, ci, h, w, co = shape
    conv = synthetic.seeded_fill_(nn.Conv2d(ci, co, k, stride=stride, padding=k // 2, padding_mode=padding_mode),
                                  seed=ci + co).to(DEV)
    x = _rand((b, ci, h, w), seed=sum(shape))
    if tf_same:
        pads = ops.tf_same_pads(h, w, k, stride)
        ho, wo = (h + pads[0] + pads[2] - k) // stride + 1, (w + pads[1] + pads[3] - k) // stride + 1
    else:
        ho, wo = ops.conv_out_hw(h, w, stride, k)
    tensors = {"x": x, "res": _rand((b, co, ho, wo), seed=sum(shape) + 1), "gate": None}
    if gate:
        tensors["gate"] = torch.rand((b, ci), generator=torch.Generator().manual_seed(3)).to(DEV)
    kw = dict(act="silu") if act == "silu" else dict(leaky=act)
    seen = []

    def op(t, out):
        y = ops.conv2d(t["x"], conv, residual=t["res"], out=out, tf_same=tf_same, gate=t["gate"], **kw)
        if ops.PROFILE:
            seen.append(ops.PROFILE[0][0])
        return y
    run_case(op, tensors, out_shape=(b, co, ho, wo), offset=offset, guard_kw=guard_kw, refuses=refuses,
             reference=_conv_ref(conv, stride, act=act, tf_same=tf_same), tol=2e-5, what=what or f"conv2d {shape}")
    if expect is not None and refuses is None and offset == 0:
        assert seen and all(s.startswith(expect) for s in seen), (what, seen, expect)


# direct 3x3 (implicit GEMM, csrc/sr_conv.hip): image layout
DIRECT = [(2, ci, 9, 11, co) for ci in (3, 30) for co in (1, 5, 130)]


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", DIRECT, ids=str)
@pytest.mark.parametrize("offset", [0, 1])
def test_direct_conv3x3(shape, stride, offset, sr_option):
    sr_option("SR_CONV_WINO", 0)
    _conv_case(shape, stride=stride, offset=offset, expect=f"sr_conv_kernel<3, {stride},")


@pytest.mark.parametrize("offset", [0, 1])
def test_conv1x1_implicit_gemm(offset, monkeypatch):
    """(3, 24, 33, 47) -> 1: an odd pixel count, so the dense run is not re-shaped into a strip and both runs take one plan."""
    monkeypatch.setattr(ops, "USE_PW_1X1", False)
    _conv_case((3, 24, 33, 47, 1), k=1, offset=offset, expect="sr_conv_kernel<1, 1,")


@pytest.mark.parametrize("ksplit", [1, 0])
def test_strided_conv_split_k(ksplit, sr_option):
    """(1, 144, 9, 7) -> 40, stride 2: partial sums in a workspace (here: freshly allocated and poisoned) + the finish."""
    assert _lib.lib().sr_conv_splitk_workspace_bytes(1, 9, 7, 144, 40, 3, 2) > 0
    sr_option("SR_CONV_KSPLIT", ksplit)
    _conv_case((1, 144, 9, 7, 40), stride=2, expect="sr_conv_kernel<3, 2,")


@pytest.mark.parametrize("offset", [0, 1])
def test_replicate_padded_conv(offset):
    _conv_case((2, 128, 10, 18, 16), padding_mode="replicate", offset=offset, expect="sr_conv_kernel<3, 1,")


@pytest.mark.parametrize("offset", [0, 1])
def test_tf_same_padded_conv(offset):
    _conv_case((1, 24, 37, 51, 96), stride=2, tf_same=True, act="silu", offset=offset, expect="sr_conv_kernel<3, 2,")


# F(2x2) Winograd (csrc/sr_wino.hip), image layout: Cin = 24 (a cut 16-channel slab), Cout = 24 (the border epilogue on every
# region), fewer regions than CUs, and a split-K plan
WINO2 = [(1, 24, 17, 23, 64), (1, 64, 20, 18, 24), (3, 48, 17, 29, 32), (1, 192, 8, 12, 32)]


@pytest.mark.parametrize("shape", WINO2, ids=str)
@pytest.mark.parametrize("offset", [0, 1])
def test_winograd_f2(shape, offset, monkeypatch, sr_option):
    sr_option("SR_CONV_WINO", 2)
    monkeypatch.setattr(ops, "WINO4_MODE", 0)
    if shape == (1, 192, 8, 12, 32):
        assert _lib.lib().sr_wino_splitk_factor(1, 8, 12, 192, 32) > 1, "the launch plan should split this shape"
    _conv_case(shape, offset=offset, expect="sr_wino_kernel<")


# F(4x4) Winograd (csrc/sr_wino4.hip), image layout, in its three kernel forms; misaligned views are handed on to F(2x2)
WINO4 = [(1, 36, 9, 7, 12), (1, 24, 35, 53, 64), (2, 16, 16, 16, 128)]


@pytest.mark.parametrize("variant", [1, 2, 3])
@pytest.mark.parametrize("shape", WINO4, ids=str)
def test_winograd_f4(shape, variant, monkeypatch, sr_option):
    sr_option("SR_CONV_WINO", 2)
    monkeypatch.setattr(ops, "WINO4_MODE", 2)
    monkeypatch.setattr(ops, "WINO4_VARIANT", variant)
    ops._SHAPE_QUERIES.clear()
    try:
        _conv_case(shape, expect={1: "sr_wino4_kernel", 2: "sr_wino4pp_kernel", 3: "sr_wino4ws_kernel"}[variant])
    finally:
        ops._SHAPE_QUERIES.clear()


def test_winograd_f4_hands_misaligned_views_on(monkeypatch, sr_option):
    sr_option("SR_CONV_WINO", 2)
    monkeypatch.setattr(ops, "WINO4_MODE", 2)
    ops._SHAPE_QUERIES.clear()
    try:
        _conv_case((1, 24, 35, 53, 64), offset=1)
    finally:
        ops._SHAPE_QUERIES.clear()


# pointwise GEMM (csrc/sr_pw.hip; image layout) and its LDS-tiled form (csrc/sr_pw_tiled.hip; image, batch-dense):
# (B, Cin, H, W, Cout, activation, gate, plan).  None of the three ragged shapes is deep enough for a K split (the plans need
# 8 / 4 K steps per split), so the split plans run on (1, 640, 15, 20) -> 384 of the same list in test_gpu_conv.PW_SHAPES.
PW = [((3, 24, 33, 47, 48), 0.0, False, None), ((2, 20, 9, 11, 1), 0.2, False, None), ((2, 64, 7, 5, 100), "silu", True, None)]
PW_DIRECT = PW + [((1, 640, 15, 20, 384), 0.2, False, (2, 4)), ((2, 64, 7, 5, 100), "silu", True, (1, 1))]
PW_TILED = PW + [((1, 640, 15, 20, 384), 0.2, False, (0, 4)), ((2, 64, 7, 5, 100), "silu", True, (3, 1))]


@pytest.mark.parametrize("shape,act,gate,plan", PW_DIRECT, ids=str)
def test_pointwise_gemm(shape, act, gate, plan, monkeypatch, sr_option):
    monkeypatch.setattr(ops, "PW_TILED", "0")
    expect = "sr_pw_kernel<"
    if plan is not None:
        sr_option("SR_PW_NT", plan[0])
        sr_option("SR_PW_KS", plan[1])
        expect = f"sr_pw_kernel<{plan[0]}, {plan[1]}"
    _conv_case(shape, k=1, act=act, gate=gate, expect=expect)


@pytest.mark.parametrize("shape,act,gate,plan", PW_TILED, ids=str)
def test_pointwise_gemm_tiled(shape, act, gate, plan, monkeypatch, sr_option):
    monkeypatch.setattr(ops, "PW_TILED", "1")
    if plan is not None:
        sr_option("SR_PT_CFG", plan[0])
        sr_option("SR_PT_KS", plan[1])
    ops._SHAPE_QUERIES.clear()
    try:
        _conv_case(shape, k=1, act=act, gate=gate, guard_kw=dict(batch_gap=0), expect="sr_pw_tiled_kernel<")
    finally:
        ops._SHAPE_QUERIES.clear()


def test_pointwise_gemm_misaligned_views(monkeypatch):
    """A misaligned input goes to the implicit-GEMM kernel; a GATED 1x1 convolution has no such kernel behind it and refuses."""
    monkeypatch.setattr(ops, "PW_TILED", "0")
    _conv_case((3, 24, 33, 47, 48), k=1, act=0.0, offset=1)
    _conv_case((2, 64, 7, 5, 100), k=1, act="silu", gate=True, offset=1,
               refuses=(_lib.HipLibraryError, "gated 1x1 convolution needs"))


# ============================================================ matching encoder kernels ====================================
# The vector-only kernels (16-byte channel quads) have no scalar instantiation: a misaligned view is refused by the library,
# and the wrapper raises.
REFUSED = (_lib.HipLibraryError, "unsupported configuration")


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_stem7x7(layout):
    """(2, 3, 50, 70): the image is read through its strides -- NCHW between `ends` bands, channels-last as an image view --
    and the 64-channel result goes into a guarded destination."""
    conv = synthetic.seeded_fill_(nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=True), seed=3).to(DEV)
    img = _rand((2, 3, 50, 70), seed=5, nhwc=layout == "channels_last")
    run_case(lambda t, out: ops.stem7x7(t["img"], conv, None, leaky=0.0, out=out), {"img": img}, out_shape=(2, 64, 25, 35),
             ends_only=("img",) if layout == "nchw" else (), what=f"stem7x7 {layout}")


@pytest.mark.parametrize("stream", [1, 0])
@pytest.mark.parametrize("shape", [(1, 12, 31, 6), (2, 4, 19, 16)], ids=str)
@pytest.mark.parametrize("offset", [0, 1])
def test_maxblurpool(shape, stream, offset, sr_option):
    sr_option("SR_POOL_STREAM", stream)
    b, c, h, w = shape
    run_case(lambda t, out: ops.maxblurpool(t["x"], out=out), {"x": _rand(shape, seed=sum(shape))},
             out_shape=(b, c, (h - 2) // 2 + 1, (w - 2) // 2 + 1), offset=offset, refuses=REFUSED if offset else None,
             what=f"maxblurpool {shape} stream={stream}")


@pytest.mark.parametrize("inplace", [False, True])
@pytest.mark.parametrize("offset", [0, 1])
def test_instance_norm(inplace, offset):
    x = _rand((1, 48, 7, 5), seed=9) * 1.7 + 0.4
    run_case(lambda t, out: ops.instance_norm(t["x"], leaky=0.2, inplace=inplace), {"x": x}, inout=("x",) if inplace else (),
             offset=offset, refuses=REFUSED if offset else None, what=f"instance_norm inplace={inplace}")


@pytest.mark.parametrize("shape", [(1, 64, 1, 3), (2, 64, 11, 19)], ids=str)
@pytest.mark.parametrize("offset", [0, 1])
def test_conv1x1_stats(shape, offset):
    conv = synthetic.seeded_fill_(nn.Conv2d(64, 128, 1), seed=6).to(DEV)
    run_case(lambda t, out: ops.conv1x1_stats(t["x"], conv, eps=1e-5), {"x": _rand(shape, seed=sum(shape)) * 1.3 + 0.2},
             offset=offset, refuses=REFUSED if offset else None, what=f"conv1x1_stats {shape}")


@pytest.mark.parametrize("mode", ["replicate", "zeros"])
@pytest.mark.parametrize("offset", [0, 1])
def test_conv3x3_c16_with_fused_norm(mode, offset):
    """x as an image view; the [B, 2, C] statistics between `ends` bands (the wrapper wants them contiguous)."""
    conv = synthetic.seeded_fill_(nn.Conv2d(64, 12, 3, padding=1, padding_mode=mode), seed=8).to(DEV)
    x = _rand((2, 64, 11, 19), seed=21) * 1.7 + 0.4
    with torch.inference_mode():
        stats = ops.instance_norm_stats(x)
    run_case(lambda t, out: ops.conv3x3_c16(t["x"], conv, in_stats=t["stats"], in_leaky=0.2), {"x": x, "stats": stats},
             offset=offset, refuses=REFUSED if offset else None, what=f"conv3x3_c16 {mode}")


def test_instance_norm_stats():
    run_case(lambda t, out: ops.instance_norm_stats(t["x"]), {"x": _rand((2, 64, 11, 19), seed=22)}, what="instance_norm_stats")


# ============================================================ image-prior encoder kernels ================================

def _bn(c, seed):
    return synthetic.seeded_fill_(nn.BatchNorm2d(c, eps=1e-3), seed=seed).eval().to(DEV)


def _se(c):
    rd = max(1, c // 24)
    return (synthetic.seeded_fill_(nn.Conv2d(c, rd, 1), seed=5).to(DEV), synthetic.seeded_fill_(nn.Conv2d(rd, c, 1), seed=6).to(DEV))


# (1, 8, 131, 5): Ho = 131 at stride 1 and 66 at stride 2, both past 64 -- the 4-row band plan of the pooled sums
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", [(1, 8, 7, 33), (1, 72, 3, 3), (1, 8, 131, 5)], ids=str)
@pytest.mark.parametrize("offset", [0, 1])
def test_dwconv3x3_with_pool(shape, stride, offset):
    """The depthwise result and the per-band pooled sums are allocated by the wrapper (poisoned here): every band of every
    channel must be written."""
    c = shape[1]
    conv = synthetic.seeded_fill_(nn.Conv2d(c, c, 3, stride=stride, padding=1, groups=c, bias=False), seed=c).to(DEV)
    bn = _bn(c, stride)

    run_case(lambda t, out: ops.dwconv3x3(t["x"], conv, bn=bn, act="silu", tf_same=True, want_pool=True),
             {"x": _rand(shape, seed=sum(shape) + stride)}, offset=offset, refuses=REFUSED if offset else None,
             what=f"dwconv3x3 {shape}/s{stride}")


@pytest.mark.parametrize("shape", [(2, 72, 3, 3), (1, 8, 7, 33)], ids=str)
def test_squeeze_excite_kernels(shape):
    """se_gate / se_gates on pooled sums between `ends` bands; se_scale_ and scale_channels_ in place on an image view, their
    pooled sums and gates between `ends` bands."""
    b, c, h, w = shape
    se_r, se_e = _se(c)
    conv = synthetic.seeded_fill_(nn.Conv2d(c, c, 3, padding=1, groups=c, bias=False), seed=c).to(DEV)
    with torch.inference_mode():
        d, pool = ops.dwconv3x3(_rand(shape, seed=4), conv, act="silu", want_pool=True)
        gate = ops.se_gate(pool, h * w, se_r, se_e)
    run_case(lambda t, out: ops.se_gate(t["pool"], h * w, se_r, se_e), {"pool": pool}, what=f"se_gate {shape}")
    run_case(lambda t, out: ops.se_gates(t["pool"], h * w, se_r, se_e), {"pool": pool}, what=f"se_gates {shape}")
    run_case(lambda t, out: ops.se_scale_(t["x"], t["pool"], se_r, se_e, want_gate=True), {"x": d, "pool": pool},
             inout=("x",), what=f"se_scale_ {shape}")
    run_case(lambda t, out: ops.scale_channels_(t["x"], t["gate"]), {"x": d, "gate": gate}, inout=("x",),
             what=f"scale_channels_ {shape}")
    run_case(lambda t, out: ops.scale_channels_(t["x"], t["gate"]), {"x": d, "gate": gate}, inout=("x",), offset=1,
             refuses=REFUSED, what=f"scale_channels_ {shape} misaligned")
    run_case(lambda t, out: ops.se_scale_(t["x"], t["pool"], se_r, se_e, want_gate=True), {"x": d, "pool": pool},
             inout=("x",), offset=1, refuses=REFUSED, what=f"se_scale_ {shape} misaligned")


@pytest.mark.parametrize("offset", [0, 1])
def test_add_on_a_slice(offset):
    y, x = _rand((2, 24, 17, 19), seed=3), _rand((2, 24, 17, 19), seed=4)
    run_case(lambda t, out: ops.add_(t["y"], t["x"]), {"y": y, "x": x}, inout=("y",), offset=offset,
             refuses=REFUSED if offset else None, what="add_")


@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
@pytest.mark.parametrize("shape", [(1, 73, 89), (1, 2, 2)], ids=str)
def test_rgb_stem3x3s2(shape, layout):
    b, h, w = shape
    conv = synthetic.seeded_fill_(nn.Conv2d(3, 24, 3, stride=2, padding=1, bias=False), seed=2).to(DEV)
    bn = _bn(24, 5)
    img = _rand((b, 3, h, w), seed=h * 3 + w, nhwc=layout == "channels_last")
    run_case(lambda t, out: ops.rgb_stem3x3s2(t["img"], conv, bn=bn, act="silu", tf_same=True), {"img": img},
             ends_only=("img",) if layout == "nchw" else (), what=f"rgb_stem3x3s2 {shape} {layout}")


@pytest.mark.parametrize("quad", [1, 0])
@pytest.mark.parametrize("shape", [(1, 16, 1, 9), (2, 12, 7, 5)], ids=str)
@pytest.mark.parametrize("offset", [0, 1])
def test_upsample2x(shape, quad, offset, sr_option):
    sr_option("SR_UPSAMPLE_QUAD", quad)
    b, c, h, w = shape
    run_case(lambda t, out: ops.upsample2x(t["x"], out=out), {"x": _rand(shape, seed=sum(shape))},
             out_shape=(b, c, 2 * h, 2 * w), offset=offset, tol=1e-6,
             reference=lambda t: F.interpolate(t["x"].double(), scale_factor=2, mode="bilinear", align_corners=False),
             what=f"upsample2x {shape} quad={quad}")


# ============================================================ 16-bit I/O entry points =====================================
# Raw C-ABI calls (what autograd_ops runs under autocast): image layout, 8 lead / tail elements = 16 bytes in 16-bit types.
DTYPES = [torch.float16, torch.bfloat16]
IO = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}


def _half_operands(shape, dt, stride=1, k=3):
    b, ci, h, w, co = shape
    ho, wo = ops.conv_out_hw(h, w, stride, k)
    conv = nn.Conv2d(ci, co, k, stride=stride, padding=k // 2)
    synthetic.seeded_fill_(conv, seed=ci + co)
    return conv.to(DEV), {"x": _rand((b, ci, h, w), seed=sum(shape)).to(dt), "res": _rand((b, co, ho, wo), seed=co).to(dt)}, \
        (b, co, ho, wo)


@pytest.mark.parametrize("dt", DTYPES, ids=str)
@pytest.mark.parametrize("shape", [(1, 24, 40, 56, 24), (3, 32, 17, 23, 96)], ids=str)
def test_winograd_16bit_io(shape, dt):
    lib = _lib.lib()
    conv, tensors, out_shape = _half_operands(shape, dt)
    b, ci, h, w, co = shape
    wp, bias = ops.packed_wino_weight(conv)

    def op(t, out):
        out = torch.empty(out_shape, dtype=dt, device=DEV).contiguous(memory_format=torch.channels_last) if out is None else out
        x, res = t["x"], t["res"]
        _lib.check(lib.sr_conv3x3_wino_io_nhwc_fwd(_lib.ptr(x), *ops._strides(x), _lib.ptr(wp), _lib.ptr(bias), _lib.ptr(res),
                                                   *ops._strides(res), _lib.ptr(out), *ops._strides(out), b, h, w, ci, co,
                                                   C.c_float(0.2), IO[dt], _lib.stream_ptr(x.device)), "wino_io")
        return out
    run_case(op, tensors, out_shape=out_shape, out_dtype=dt, what=f"wino 16-bit io {shape} {dt}")


@pytest.mark.parametrize("dt", DTYPES, ids=str)
@pytest.mark.parametrize("shape", [(1, 64, 33, 47, 1), (3, 112, 12, 20, 100)], ids=str)
def test_pointwise_16bit_io(shape, dt):
    lib = _lib.lib()
    conv, tensors, out_shape = _half_operands(shape, dt, k=1)
    b, ci, h, w, co = shape
    wp, bias = ops.packed_weight(conv)

    def op(t, out):
        out = torch.empty(out_shape, dtype=dt, device=DEV).contiguous(memory_format=torch.channels_last) if out is None else out
        x, res = t["x"], t["res"]
        _lib.check(lib.sr_pw_conv_io_nhwc_fwd(_lib.ptr(x), *ops._strides(x), _lib.ptr(wp), _lib.ptr(bias), _lib.ptr(res),
                                              *ops._strides(res), _lib.ptr(out), *ops._strides(out), b, h * w, ci, co,
                                              C.c_float(0.2), IO[dt], _lib.stream_ptr(x.device)), "pw_io")
        return out
    run_case(op, tensors, out_shape=out_shape, out_dtype=dt, what=f"pointwise 16-bit io {shape} {dt}")


@pytest.mark.parametrize("dt", DTYPES, ids=str)
@pytest.mark.parametrize("k,stride", [(1, 1), (3, 1), (3, 2)])
@pytest.mark.parametrize("shape", [(1, 8, 5, 7, 8), (3, 24, 17, 23, 40), (1, 40, 6, 9, 64)], ids=str)
def test_conv16_mfma(shape, k, stride, dt):
    """sr_conv16_nhwc_fwd at the three forms of test_gpu_conv16.FORMS, Cin in {8, 24, 40}; 16-bit output, and fp32 output
    for the Cin = 24 shape."""
    lib = _lib.lib()
    conv, tensors, out_shape = _half_operands(shape, dt, stride=stride, k=k)
    b, ci, h, w, co = shape
    odt = torch.float32 if ci == 24 else dt
    wp = torch.zeros(lib.sr_conv16_packed_weight_bytes(co, ci, k), dtype=torch.uint8, device=DEV)
    _lib.check(lib.sr_conv16_pack_weights(_lib.ptr(conv.weight.detach().contiguous()), co, ci, k, IO[dt], _lib.ptr(wp),
                                          _lib.stream_ptr(wp.device)), "sr_conv16_pack_weights")
    bias = conv.bias.detach()

    def op(t, out):
        out = torch.empty(out_shape, dtype=odt, device=DEV).contiguous(memory_format=torch.channels_last) if out is None else out
        x, res = t["x"], t["res"]
        _lib.check(lib.sr_conv16_nhwc_fwd(_lib.ptr(x), *ops._strides(x), _lib.ptr(wp), _lib.ptr(bias), _lib.ptr(res),
                                          *ops._strides(res), _lib.ptr(out), *ops._strides(out), b, h, w, ci, co, k, stride,
                                          C.c_float(0.2), IO[dt], IO[odt], _lib.stream_ptr(x.device)), "sr_conv16_nhwc_fwd")
        return out
    run_case(op, tensors, out_shape=out_shape, out_dtype=odt, what=f"conv16 {shape} k{k} s{stride} {dt}")


# ============================================================ training kernels =============================================
# Through autograd_ops / train_ops: the forward input (read again by the weight-gradient kernels) as an image view, the
# incoming gradient as an image view too (the wrappers make a dense copy of a strided gradient: the copy is theirs, and
# allocated poisoned here).

def _backward_case(fn, tensors, params=(), leaves=("x",), **kw):
    """y = fn(t) with t[leaf] requiring grad; y.backward(t["g"]) -> (y, d leaf ..., d param ...)."""
    def op(t, out):
        t = dict(t)
        for k in leaves:
            t[k] = t[k].detach().requires_grad_()
        for p in params:
            p.grad = None
        y = fn(t)
        y.backward(t["g"])
        return (y.detach(),) + tuple(t[k].grad for k in leaves) + tuple(p.grad.clone() for p in params)
    run_case(op, tensors, grad=True, **kw)


@pytest.mark.parametrize("name", ["seg_edges_w33", "rgb_in", "few_per"])
def test_conv_backward(name):
    """bwd_cases.CONV_CASES: a 3x3 / stride 1 (Winograd data gradient, residual, LeakyReLU), a 3x3 / stride 2 TF-"SAME" with
    3 input channels, and a 1x1 with 196 (co, ci) blocks: weight, data, bias and residual gradients and the fused
    activation + bias backward."""
    import bwd_cases as bc
    from simplerecon_amd import train_ops
    case = bc.CONV_BY_NAME[name]
    geo = bc.conv_geometry(case)
    inp = bc.conv_inputs(case, DEV)
    conv = nn.Conv2d(case["ci"], case["co"], case["k"], stride=case["s"], padding=case["k"] // 2, bias=True).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(inp["w"])
        conv.bias.copy_(inp["b"] if inp["b"] is not None else torch.linspace(-0.1, 0.1, case["co"]))
    tensors = {"x": inp["xw"], "g": inp["Rw"], "res": inp["res"]}
    leaves = ("x", "res") if inp["res"] is not None else ("x",)
    _backward_case(lambda t: train_ops.conv(t["x"], conv, pads=geo["pads"], residual=t["res"], slope=0.2), tensors,
                   params=(conv.weight, conv.bias), leaves=leaves, what=f"conv backward {name}")


@pytest.mark.parametrize("mode", ["bn_train_silu", "bn_eval_relu", "in_leaky"])
@pytest.mark.parametrize("shape", [(2, 48, 7, 5), (2, 30, 6, 5)], ids=str)
def test_norm_act_backward(shape, mode):
    """(2, 30, 6, 5): C % 4 != 0, the scalar instantiation."""
    import bwd_cases as bc
    from simplerecon_amd import train_ops
    c = shape[1]
    bn = synthetic.seeded_fill_(nn.BatchNorm2d(c, eps=1e-3), seed=c).to(DEV)
    bn.train(mode == "bn_train_silu")
    tensors = {"x": _rand(shape, seed=1) * 1.5 + 0.3, "g": _rand(shape, seed=2)}
    if mode == "in_leaky":
        _backward_case(lambda t: train_ops.instance_norm_act(t["x"], leaky=0.2), tensors, what=f"instance_norm_act {shape}")
    else:
        act = bc.ACT_SILU if mode == "bn_train_silu" else 0.0
        _backward_case(lambda t: train_ops.batch_norm_act(t["x"], bn, act=act), tensors, params=(bn.weight, bn.bias),
                       what=f"batch_norm_act {mode} {shape}")


def test_maxblurpool_backward_small_maps():
    import bwd_cases as bc
    from simplerecon_amd import train_ops
    for h, w in bc.MBP_SMALL:
        x = bc.tie_input("relu_zeros", (2, 8, h, w), seed=h * 7 + w).to(DEV).contiguous(memory_format=torch.channels_last)
        g = _rand((2, 8, (h - 2) // 2 + 1, (w - 2) // 2 + 1), seed=h + w)
        _backward_case(lambda t: train_ops.maxblurpool(t["x"]), {"x": x, "g": g}, what=f"maxblurpool backward {h}x{w}")


@pytest.mark.parametrize("shape,stride", [((1, 8, 7, 33), 2), ((1, 72, 3, 3), 1)], ids=str)
def test_depthwise_backward(shape, stride):
    from simplerecon_amd import train_ops
    b, c, h, w = shape
    conv = synthetic.seeded_fill_(nn.Conv2d(c, c, 3, stride=stride, padding=1, groups=c, bias=False), seed=c).to(DEV)
    pads = ops.tf_same_pads(h, w, 3, stride)
    ho, wo = (h + pads[0] + pads[2] - 3) // stride + 1, (w + pads[1] + pads[3] - 3) // stride + 1
    _backward_case(lambda t: train_ops.dwconv3x3(t["x"], conv, pads), {"x": _rand(shape, seed=5), "g": _rand((b, c, ho, wo), seed=6)},
                   params=(conv.weight,), what=f"dwconv3x3 backward {shape}/s{stride}")


def test_upsample2x_backward():
    from simplerecon_amd import autograd_ops
    _backward_case(lambda t: autograd_ops.upsample2x(t["x"]), {"x": _rand((3, 12, 37, 53), seed=7), "g": _rand((3, 12, 74, 106), seed=8)},
                   what="upsample2x backward")


# ============================================================ plane sweeps =================================================
# The managers make their operands contiguous and take no strided view: `ends` bands on every operand (features, poses,
# intrinsics, depth planes, depth range, and the cotangent of the backward pass).

def _sweep_case(mgr, inp, cot, loose, what, return_mask=False):
    tensors = dict(inp)
    tensors["g"] = cot
    keys = list(inp)
    params = [p for p in mgr.parameters()]

    def op(t, out):
        t = dict(t)
        g = t.pop("g")
        for k in ("cur_feats", "src_feats"):
            t[k] = t[k].detach().requires_grad_()
        for p in params:
            p.grad = None
        vol, lowest, _, mask = mgr(**t, **({"return_mask": True} if return_mask else {}))
        vol.backward(g)
        return (vol.detach(), lowest, mask, t["cur_feats"].grad, t["src_feats"].grad) + tuple(p.grad.clone() for p in params)
    with torch.inference_mode():
        fwd = lambda t, out: mgr(**{k: t[k] for k in keys}, **({"return_mask": True} if return_mask else {}))[:2]
        run_case(fwd, dict(inp), ends_only=keys, what=what + " forward")
    run_case(op, tensors, ends_only=list(tensors), grad=True, loose=loose, what=what + " forward + backward")
    mgr._workspace = None


@pytest.mark.parametrize("name", ["edge_k4", "layouts", "k1"])
def test_mlp_sweep(name):
    """volume_cases.EDGE_CASE / LAYOUT_CASE / k1.  Bit-equal: volume, lowest cost, mask; the gradients are scattered with
    atomics (outputs 3 ...)."""
    import volume_cases as vc
    case = {c["name"]: c for c in vc.SMALL_CASES}[name]
    inp = vc.to_device(vc.inputs(case), DEV)
    mgr = vc.manager(case).to(DEV)
    cot = torch.from_numpy(vc.cotangent(case)).to(DEV)
    _sweep_case(mgr, inp, cot, loose=tuple(range(3, 5 + len(list(mgr.parameters())))), what=f"MLP sweep {name}", return_mask=True)


@pytest.mark.parametrize("lds", [1, 0])
@pytest.mark.parametrize("C", [12, 32])
def test_dot_sweep(C, lds, sr_option):
    """volume_cases.DOT_SHAPES["spread"], LDS-staged and L1-gather forms.  d cur_feats is accumulated in registers (bit-equal);
    d src_feats is scattered with atomics (output 4)."""
    import volume_cases as vc
    from simplerecon_amd.cost_volume import CostVolumeManager
    shape = vc.DOT_SHAPES["spread"]
    sr_option("SR_DOT_LDS", lds)
    inp = vc.to_device(vc.dot_inputs(shape, C), DEV)
    mgr = CostVolumeManager(shape["h"], shape["w"], num_depth_bins=shape["D"], matching_dim_size=C).to(DEV)
    cot = torch.from_numpy(vc.cotangent(shape)).to(DEV)
    _sweep_case(mgr, inp, cot, loose=(4,), what=f"dot sweep C={C} lds={lds}")


def test_warp_features():
    import volume_cases as vc
    from simplerecon_amd.cost_volume import CostVolumeManager
    case = vc.WARP_CASE
    b, k, c, d, h, w = (case[x] for x in ("B", "K", "C", "D", "h", "w"))
    inp = vc.to_device(vc.inputs(case), DEV)
    mgr = CostVolumeManager(h, w, num_depth_bins=d, matching_dim_size=c).to(DEV)
    tensors = {"src_feats": inp["src_feats"], "src_extrinsics": inp["src_extrinsics"], "src_Ks": inp["src_Ks"],
               "cur_invK": inp["cur_invK"], "plane": inp["depth_planes_bdhw"][:, d - 1].unsqueeze(1).contiguous()}
    run_case(lambda t, out: mgr.warp_features(t["src_feats"], t["src_extrinsics"], t["src_Ks"], t["cur_invK"], t["plane"],
                                              b, k, c, None), tensors, ends_only=list(tensors), what="warp_features")
