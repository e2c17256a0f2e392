"""What the convolution entry points refuse, asked through the C ABI with made-up addresses: every case here is turned away
by host code BEFORE the first HIP call (csrc/sr_view.h holds the rules), so nothing is launched and no GPU is needed -- and
none of the addresses is ever dereferenced where one is present.  A call the library ACCEPTS would launch on these
addresses: such a call is not a case (sr_conv3x3_wino_nhwc_fwd takes a misaligned fp32 input through its scalar
instantiation, sr_pw_conv_nhwc_fwd stores single elements and takes any output / residual alignment, the tiled GEMM
addresses flat and has no span limit)."""
import pytest

from simplerecon_amd import _lib

INVALID, UNSUPPORTED = 1, 2
IN, WP, BIAS, RES, OUT, GATE, WS = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000, 0x700000
OFF = 4   # bytes: off a 16-byte and off an 8-byte boundary alike

# A 4096 x 4096 map has 2^24 pixels: at a pixel stride of 36 elements an image spans 2.4e9 bytes, past the 2^31 that 32-bit
# buffer addressing takes; at 16 it spans 2^30.  (The boundary itself, on both sides: tests/host/view_checks.c.)
BIG_H = BIG_W = 4096
BIG_HW = BIG_H * BIG_W


def _conv3x3(name, extra=()):
    """Caller for the 3x3 entry points (wino4, its variant form, wino, wino_io): keyword overrides on a view every kernel
    form would take."""
    fn = getattr(_lib.lib(), name)

    def call(in_=IN, wp=WP, bias=BIAS, res=RES, out=OUT, B=2, H=8, W=8, Cin=16, Cout=16, in_sp=None, out_sp=None, res_sp=None,
             in_sb=None, out_sb=None, res_sb=None, tail=extra):
        in_sp, out_sp, res_sp = in_sp or Cin, out_sp or Cout, res_sp or Cout
        in_sb = H * W * in_sp if in_sb is None else in_sb
        out_sb = H * W * out_sp if out_sb is None else out_sb
        res_sb = H * W * res_sp if res_sb is None else res_sb
        return fn(in_, in_sb, in_sp, wp, bias, res, res_sb, res_sp, out, out_sb, out_sp, B, H, W, Cin, Cout, 0.0, *tail, None)
    return call


def _big(which):
    """Arguments under which exactly the `which` tensor of a 4096 x 4096 map spans more than 2^31 bytes (the others 2^30)."""
    return {"B": 1, "H": BIG_H, "W": BIG_W, "Cin": 16, "Cout": 16, which + "_sp": 36}


VECTOR_ONLY = [   # entry points whose only instantiation is the vector one: every misalignment is a refusal
    ("sr_conv3x3_wino4_nhwc_fwd", ()),
    ("sr_conv3x3_wino4_variant_nhwc_fwd", (1,)),
    ("sr_conv3x3_wino4_variant_nhwc_fwd", (2,)),
    ("sr_conv3x3_wino4_variant_nhwc_fwd", (3,)),
    ("sr_conv3x3_wino_io_nhwc_fwd", (1,)),
    ("sr_conv3x3_wino_io_nhwc_fwd", (2,)),
]
MISALIGNED = [dict(in_=IN + OFF), dict(out=OUT + OFF), dict(res=RES + OFF), dict(bias=BIAS + OFF),
              dict(in_sp=18), dict(out_sp=18), dict(res_sp=18),                  # pixel stride C + 2
              dict(in_sb=8 * 8 * 16 + 2), dict(out_sb=8 * 8 * 16 + 2), dict(res_sb=8 * 8 * 16 + 2),
              dict(Cin=6, in_sp=8), dict(Cout=6, out_sp=8, res_sp=8)]


@pytest.mark.parametrize("name,extra", VECTOR_ONLY)
def test_vector_only_3x3_entry_points(name, extra):
    call = _conv3x3(name, extra)
    for kw in (dict(in_=None), dict(wp=None), dict(out=None)):
        assert call(**kw) == INVALID, kw
    for kw in MISALIGNED:
        assert call(**kw) == UNSUPPORTED, kw
    for which in ("in", "out", "res"):
        assert call(**_big(which)) == UNSUPPORTED, which
    assert call(B=1, H=16384, W=16384, Cin=8, Cout=8) == UNSUPPORTED


def test_wino4_variant_number_is_checked_first():
    call = _conv3x3("sr_conv3x3_wino4_variant_nhwc_fwd")
    assert call(tail=(4,)) == INVALID and call(tail=(-1,)) == INVALID


def test_wino_io_dtype_is_checked_first():
    call = _conv3x3("sr_conv3x3_wino_io_nhwc_fwd")
    assert call(tail=(3,)) == INVALID and call(tail=(-1,)) == INVALID


def test_wino_fp32_refuses_null_and_spans_only():
    """(a misaligned fp32 view is ACCEPTED here -- the scalar instantiation -- and therefore not a case)"""
    call = _conv3x3("sr_conv3x3_wino_nhwc_fwd")
    for kw in (dict(in_=None), dict(wp=None), dict(out=None)):
        assert call(**kw) == INVALID, kw
    for which in ("in", "out", "res"):
        assert call(**_big(which)) == UNSUPPORTED, which
    assert call(B=1, H=16384, W=16384, Cin=8, Cout=8) == UNSUPPORTED


@pytest.mark.parametrize("fmt", [1, 2])
def test_wino_split_format_has_the_vector_instantiation_only(fmt, sr_option):
    """split_format 1 / 2 on the split-K entry point selects the split-precision kernel: what the scalar instantiation would
    take is refused, with the option that used to select the kernel off or on another mode -- the argument alone decides."""
    for option in (0, 3 - fmt):
        sr_option("SR_WINO_SPLIT", option)
        for ws in ((None, 0), (WS, 1 << 20)):
            call = _conv3x3("sr_conv3x3_wino_splitk_nhwc_fwd", (fmt, *ws))
            for kw in (dict(in_=None), dict(wp=None), dict(out=None)):
                assert call(**kw) == INVALID, kw
            for kw in MISALIGNED:
                assert call(**kw) == UNSUPPORTED, kw
            for which in ("in", "out", "res"):
                assert call(**_big(which)) == UNSUPPORTED, which


def test_wino_split_format_is_checked_before_anything_is_launched(sr_option):
    """A split_format outside 0..2 is an invalid argument of the pack and of the launch, whatever the option says."""
    for option in (0, 2):
        sr_option("SR_WINO_SPLIT", option)
        for fmt in (3, -1):
            assert _conv3x3("sr_conv3x3_wino_splitk_nhwc_fwd", (fmt, WS, 1 << 20))() == INVALID
            assert _lib.lib().sr_wino_pack_weights(IN, 16, 16, fmt, WP, None) == INVALID


def _pw(io):
    lib = _lib.lib()

    def call(in_=IN, wp=WP, bias=BIAS, gate=None, res=RES, out=OUT, B=2, HW=64, Cin=16, Cout=16, in_sp=None, out_sp=None,
             res_sp=None, in_sb=None, io_dtype=io):
        in_sp, out_sp, res_sp = in_sp or Cin, out_sp or Cout, res_sp or Cout
        in_sb = HW * in_sp if in_sb is None else in_sb
        if io is None:
            return lib.sr_pw_conv_nhwc_fwd(in_, in_sb, in_sp, wp, bias, gate, res, HW * res_sp, res_sp, out, HW * out_sp, out_sp,
                                           B, HW, Cin, Cout, 0.0, None)
        return lib.sr_pw_conv_io_nhwc_fwd(in_, in_sb, in_sp, wp, bias, res, HW * res_sp, res_sp, out, HW * out_sp, out_sp, B, HW,
                                          Cin, Cout, 0.0, io_dtype, None)
    return call


@pytest.mark.parametrize("io", [None, 1, 2])
def test_pointwise_entry_points(io):
    """The pointwise GEMM loads 4-channel input fragments and stores single elements: the INPUT side has the alignment rules."""
    call = _pw(io)
    for kw in (dict(in_=None), dict(wp=None), dict(out=None)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(in_=IN + OFF), dict(in_sp=18), dict(in_sb=64 * 16 + 2), dict(Cin=6, in_sp=8)):
        assert call(**kw) == UNSUPPORTED, kw
    for which in ("in", "out", "res"):
        assert call(B=1, HW=BIG_HW, **{which + "_sp": 36}) == UNSUPPORTED, which
    assert call(B=1, HW=16384 * 16384, Cin=8, Cout=8) == UNSUPPORTED
    if io is None:
        assert call(gate=GATE + OFF) == UNSUPPORTED
    else:
        assert call(io_dtype=3) == INVALID and call(io_dtype=-1) == INVALID


def test_tiled_pointwise_entry_point():
    fn = _lib.lib().sr_pw_conv_tiled_nhwc_fwd

    def call(in_=IN, wp=WP, gate=None, out=OUT, Cin=16, in_sp=16):
        return fn(in_, in_sp, wp, BIAS, gate, RES, 16, out, 16, 128, 64, Cin, 16, 0.0, WS, 1 << 20, None)
    for kw in (dict(in_=None), dict(wp=None), dict(out=None)):
        assert call(**kw) == INVALID, kw
    for kw in (dict(in_=IN + OFF), dict(in_sp=18), dict(Cin=6, in_sp=8), dict(gate=GATE + OFF)):
        assert call(**kw) == UNSUPPORTED, kw
