"""Host side of the 16-bit MFMA convolutions (csrc/sr_conv16.hip, SR_AUTOCAST_MFMA16): the C ABI's pure host functions and
the routing predicate of autograd_ops.  No launch: runs without a GPU."""
import ctypes as C
import os
import re

import pytest

from simplerecon_amd import _lib, autograd_ops, experimental

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_i, _p, _i64, _f, _sz = C.c_int, C.c_void_p, C.c_int64, C.c_float, C.c_size_t
EXPECTED = {
    "sr_conv16_packed_weight_bytes": (_sz, [_i, _i, _i]),
    "sr_conv16_pack_weights": (_i, [_p, _i, _i, _i, _i, _p, _p]),
    "sr_conv16_supported": (_i, [_i] * 7),
    "sr_conv16_prefers": (_i, [_i] * 7),
    "sr_conv16_nhwc_fwd": (_i, [_p, _i64, _i, _p, _p, _p, _i64, _i, _p, _i64, _i] + [_i] * 7 + [_f, _i, _i, _p]),
}


def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "simplerecon_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name, sig in EXPECTED.items():
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in the header"
        assert hasattr(raw, name), f"{name} is not exported"
        assert _lib.SIGNATURES[name] == sig, name
    # the header states the numeric contract
    sec = hdr[hdr.index("16-bit MFMA convolutions"):]
    for phrase in ("round to nearest even", "fp32 on the matrix pipe", "Subnormals", "NOT measured", "Cout % 8 == 0",
                   "SR_ERR_UNSUPPORTED", "SR_ERR_INVALID_ARGUMENT"):
        assert phrase in sec, phrase


@pytest.mark.parametrize("co,ci,k", [(8, 8, 1), (8, 8, 3), (40, 24, 3), (160, 64, 3), (128, 256, 1), (64, 40, 3), (1, 1, 1)])
def test_packed_weight_bytes(co, ci, k):
    n = _lib.lib().sr_conv16_packed_weight_bytes(co, ci, k)
    assert n >= 2 * co * ci * k * k and n % 16 == 0
    assert n <= 2 * (co + 31) * (ci + 15) * k * k        # (padding to whole 32 x 16 fragments, no more)


def test_packed_weight_bytes_of_a_bad_kernel_size_is_zero():
    assert _lib.lib().sr_conv16_packed_weight_bytes(8, 8, 5) == 0


def test_supported_truth_table():
    sup = _lib.lib().sr_conv16_supported
    assert sup(1, 16, 16, 4, 8, 3, 1) == 0
    assert sup(1, 16, 16, 8, 8, 3, 1) == 1
    assert sup(1, 16, 16, 24, 8, 3, 1) == 1
    assert sup(1, 16, 16, 8, 8, 5, 1) == 0
    assert sup(1, 16, 16, 8, 8, 1, 2) == 0
    assert sup(1, 16, 16, 8, 8, 1, 1) == 1 and sup(2, 17, 23, 8, 40, 3, 2) == 1
    assert sup(1, 16, 16, 8, 12, 3, 1) == 0               # whole 4-channel output quads of a Cout % 8 == 0 row: no scalar tail
    assert sup(0, 16, 16, 8, 8, 3, 1) == 0 and sup(1, 0, 16, 8, 8, 3, 1) == 0 and sup(1, 16, 16, 8, 8, 3, 3) == 0


def test_prefers_implies_supported():
    lib = _lib.lib()
    for b in (1, 2, 8):
        for h, w in ((240, 320), (120, 160), (60, 80), (30, 40), (15, 20)):
            for ci, co in ((64, 64), (128, 128), (256, 128), (128, 64), (12, 16), (8, 8)):
                for k, s in ((3, 1), (3, 2), (1, 1), (1, 2), (5, 1)):
                    if lib.sr_conv16_prefers(b, h, w, ci, co, k, s):
                        assert lib.sr_conv16_supported(b, h, w, ci, co, k, s)


def test_argument_errors_come_before_any_launch():
    """NULL pointers, dtypes, k and stride are refused by host code (no device needed: nothing is launched)."""
    fwd = _lib.lib().sr_conv16_nhwc_fwd
    ok = dict(io=1, out=1, k=3, s=1)

    def rc(in_=256, wp=512, out_=1024, **kw):
        a = {**ok, **kw}
        return fwd(in_, 8 * 8 * 8, 8, wp, None, None, 0, 0, out_, 8 * 8 * 8, 8, 1, 8, 8, 8, 8, a["k"], a["s"], -1.0, a["io"],
                   a["out"], None)
    for kw in (dict(io=0), dict(io=3), dict(io=2, out=1), dict(out=2), dict(k=5), dict(k=2), dict(s=3), dict(s=0),
               dict(k=1, s=2), dict(in_=None), dict(wp=None), dict(out_=None)):
        assert rc(**kw) == 1, kw                           # SR_ERR_INVALID_ARGUMENT
    assert rc(in_=264) == 2 and rc(out_=1032) == 2 and rc(wp=520) == 2      # SR_ERR_UNSUPPORTED: not 16-byte aligned
    pack = _lib.lib().sr_conv16_pack_weights
    assert pack(None, 8, 8, 3, 1, 512, None) == 1 and pack(256, 8, 8, 3, 0, 512, None) == 1 and pack(256, 8, 8, 2, 1, 512, None) == 1


def test_switch_defaults_off_and_the_predicate_never_selects_at_zero(monkeypatch):
    assert os.environ.get("SR_AUTOCAST_MFMA16", "0") != "0" or autograd_ops.MFMA16 == 0
    monkeypatch.setattr(autograd_ops, "MFMA16", 0)
    shapes = [(b, h, w, ci, co, k, s) for b in (1, 2, 8) for h, w in ((240, 320), (60, 80), (15, 20))
              for ci, co in ((64, 64), (256, 128), (8, 8)) for k, s in ((3, 1), (3, 2), (1, 1))]
    assert not any(autograd_ops._mfma16_selects(*sh, None) for sh in shapes)
    monkeypatch.setattr(autograd_ops, "MFMA16", 2)
    assert all(autograd_ops._mfma16_selects(*sh, None) for sh in shapes)
    assert not autograd_ops._mfma16_selects(2, 60, 80, 64, 64, 3, 1, (1, 1, 1, 1))       # explicit pads keep their path
    assert not autograd_ops._mfma16_selects(2, 60, 80, 12, 16, 3, 1, None)
    monkeypatch.setattr(autograd_ops, "MFMA16", 1)
    lib = _lib.lib()
    for sh in shapes:
        assert autograd_ops._mfma16_selects(*sh, None) == bool(lib.sr_conv16_prefers(*sh))


def test_context_manager_sets_and_restores_the_three_switches(monkeypatch):
    monkeypatch.setattr(autograd_ops, "HALF_IO", False)
    monkeypatch.setattr(autograd_ops, "STORE_HALF", False)
    monkeypatch.setattr(autograd_ops, "MFMA16", 0)
    with experimental.autocast_mfma16():
        assert (autograd_ops.HALF_IO, autograd_ops.MFMA16, autograd_ops.STORE_HALF) == (True, 1, True)
        with experimental.autocast_mfma16(mode=2, storage=False):
            assert (autograd_ops.HALF_IO, autograd_ops.MFMA16, autograd_ops.STORE_HALF) == (True, 2, True)
        assert autograd_ops.MFMA16 == 1
    assert (autograd_ops.HALF_IO, autograd_ops.MFMA16, autograd_ops.STORE_HALF) == (False, 0, False)
    with pytest.raises(RuntimeError):
        with experimental.autocast_mfma16(mode=2, storage=False):
            assert (autograd_ops.HALF_IO, autograd_ops.MFMA16, autograd_ops.STORE_HALF) == (True, 2, False)
            raise RuntimeError("leave through an exception")
    assert (autograd_ops.HALF_IO, autograd_ops.MFMA16, autograd_ops.STORE_HALF) == (False, 0, False)
    with pytest.raises(ValueError):
        with experimental.autocast_mfma16(mode=3):
            pass
    assert "process-wide" in experimental.autocast_mfma16.__doc__
