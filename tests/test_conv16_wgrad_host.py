"""Host side of the 16-bit weight gradient (csrc/sr_conv16_wgrad.hip, SR_AUTOCAST_MFMA16_WGRAD): the C ABI's pure host
functions, the context manager and the routing predicate of autograd_ops.  No launch: runs without a GPU."""
import ctypes as C
import os
import re

import pytest

from simplerecon_amd import _lib, autograd_ops, experimental

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_i, _p, _i64, _f, _sz = C.c_int, C.c_void_p, C.c_int64, C.c_float, C.c_size_t
EXPECTED = {
    "sr_conv16_wgrad_supported": (_i, [_i] * 7),
    "sr_conv16_wgrad_prefers": (_i, [_i] * 7),
    "sr_conv16_wgrad_workspace_bytes": (_sz, [_i] * 7),
    "sr_conv16_wgrad_nhwc": (_i, [_p, _i64, _i, _p, _i64, _i, _p] + [_i] * 8 + [_p, _sz, _p]),
    "sr_act_bwd_bias16_workspace_bytes": (_sz, [_i64, _i]),
    "sr_act_bwd_bias16_nhwc": (_i, [_p, _i, _p, _p, _p, _i64, _i, _f, _i, _p, _sz, _p]),
}
GRID = [(b, h, w, ci, co, k, s) for b in (-1, 0, 1, 2, 8) for h, w in ((240, 320), (33, 64), (17, 23), (4, 45), (1, 1), (0, 16))
        for ci, co in ((64, 64), (256, 128), (8, 8), (24, 40), (12, 16), (8, 12), (4, 8), (64, 160))
        for k, s in ((3, 1), (3, 2), (1, 1), (1, 2), (5, 1), (3, 3), (2, 1))]


def expected_workspace_bytes(b, h, w, ci, co, k, s):
    """The formula include/simplerecon_hip.h documents: (blocks, slabs per block, bytes)."""
    pad = k // 2
    ho, wo = (h + 2 * pad - k) // s + 1, (w + 2 * pad - k) // s + 1
    blocks = -(-co // 64) * -(-ci // 64)
    slabs = min(-(-512 // blocks), b * ho * -(-wo // 32))
    return blocks, slabs, blocks * slabs * k * k * 64 * 64 * 4


def test_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "simplerecon_hip.h")).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for name, sig in EXPECTED.items():
        assert re.search(r"\b" + name + r"\s*\(", hdr), f"{name} is not declared in the header"
        assert hasattr(raw, name), f"{name} is not exported"
        assert _lib.SIGNATURES[name] == sig, name
    # the header states the numeric contract and the workspace formula
    sec = hdr[hdr.index("16-bit-operand weight gradient"):]
    for phrase in ("products of two 16-bit values are exact", "fp32 on the matrix pipe", "function of the shape only",
                   "no atomics", "NOT rounded", "blocks x slabs x k k x 64 x 64 x 4", "ceil(512 / blocks)", "Cout % 8 == 0",
                   "SR_ERR_UNSUPPORTED", "SR_ERR_INVALID_ARGUMENT", "64-bit"):
        assert phrase in sec, phrase


def test_supported_agrees_with_the_forward_kernel_on_form_and_channel_rules():
    lib = _lib.lib()
    seen = set()
    for sh in GRID:
        got = lib.sr_conv16_wgrad_supported(*sh)
        assert got == lib.sr_conv16_supported(*sh), sh
        if sh[0] <= 0:
            assert got == 0, sh
        seen.add(got)
    assert seen == {0, 1}
    sup = lib.sr_conv16_wgrad_supported
    assert sup(1, 16, 16, 8, 8, 3, 1) == 1 and sup(1, 16, 16, 8, 8, 3, 2) == 1 and sup(1, 16, 16, 8, 8, 1, 1) == 1
    assert sup(1, 16, 16, 12, 8, 3, 1) == 0 and sup(1, 16, 16, 8, 12, 3, 1) == 0 and sup(1, 16, 16, 8, 8, 1, 2) == 0
    assert sup(1, 16, 16, 8, 8, 5, 1) == 0 and sup(1, 16, 16, 8, 8, 3, 3) == 0 and sup(0, 16, 16, 8, 8, 3, 1) == 0


def test_prefers_implies_supported():
    lib = _lib.lib()
    for sh in GRID:
        if lib.sr_conv16_wgrad_prefers(*sh):
            assert lib.sr_conv16_wgrad_supported(*sh), sh


def test_workspace_bytes_follow_the_documented_formula():
    lib = _lib.lib()
    n_checked = 0
    for sh in GRID:
        n = lib.sr_conv16_wgrad_workspace_bytes(*sh)
        if not lib.sr_conv16_wgrad_supported(*sh):
            assert n == 0, sh
            continue
        blocks, slabs, want = expected_workspace_bytes(*sh)
        assert n == want and n % 16 == 0 and slabs >= 1, (sh, n, want)
        n_checked += 1
    assert n_checked > 50
    for px, c in ((35, 8), (1000, 40), (1, 8), (2 * 240 * 320, 64), (10 ** 7, 256)):
        n = lib.sr_act_bwd_bias16_workspace_bytes(px, c)
        assert n % 16 == 0 and n >= 4 * c and n % (4 * c) == 0, (px, c, n)
    assert lib.sr_act_bwd_bias16_workspace_bytes(35, 12) == 0 and lib.sr_act_bwd_bias16_workspace_bytes(0, 8) == 0


def test_argument_errors_come_before_any_launch():
    """NULL pointers, dtypes, k and stride are refused by host code (no device needed: nothing is launched)."""
    lib = _lib.lib()
    ok = dict(io=1, k=3, s=1, ci=8, co=8)

    def rc(in_=256, g=512, dw=1024, ws=2048, nws=1 << 30, sp=None, **kw):
        a = {**ok, **kw}
        return lib.sr_conv16_wgrad_nhwc(in_, 8 * 8 * 16, 16 if sp is None else sp, g, 8 * 8 * 16, 16, dw, 1, 8, 8, a["ci"], a["co"],
                                        a["k"], a["s"], a["io"], ws, nws, None)
    for kw in (dict(io=0), dict(io=3), dict(k=5), dict(k=2), dict(s=3), dict(s=0), dict(k=1, s=2), dict(in_=None), dict(g=None),
               dict(dw=None), dict(ws=None)):
        assert rc(**kw) == 1, kw                           # SR_ERR_INVALID_ARGUMENT
    need = lib.sr_conv16_wgrad_workspace_bytes(1, 8, 8, 8, 8, 3, 1)
    for kw in (dict(in_=264), dict(g=520), dict(ws=2056), dict(ci=12), dict(co=12), dict(sp=20), dict(sp=4), dict(nws=need - 1)):
        assert rc(**kw) == 2, kw                           # SR_ERR_UNSUPPORTED
    act = lib.sr_act_bwd_bias16_nhwc
    assert act(256, 0, 512, 1024, None, 35, 8, 0.2, 0, None, 0, None) == 1          # io_dtype 0
    assert act(256, 2, 512, 1024, None, 35, 8, 0.2, 1, None, 0, None) == 1          # bf16 gradient of an fp16 layer
    assert act(None, 1, 512, 1024, None, 35, 8, 0.2, 1, None, 0, None) == 1
    assert act(256, 1, 512, None, None, 35, 8, 0.2, 1, None, 0, None) == 1          # an activation needs grad_pre
    assert act(256, 1, 512, 1024, None, 35, 8, -0.5, 1, None, 0, None) == 1
    assert act(256, 1, 512, 1024, None, 35, 12, 0.2, 1, None, 0, None) == 2         # C % 8
    assert act(264, 1, 512, 1024, None, 35, 8, 0.2, 1, None, 0, None) == 2          # 8 bytes off
    assert act(256, 1, 512, 1024, 4096, 35, 8, 0.2, 1, 8192, 0, None) == 3          # SR_ERR_WORKSPACE_TOO_SMALL


def test_switch_defaults_off_and_the_predicate_never_selects_at_zero(monkeypatch):
    assert os.environ.get("SR_AUTOCAST_MFMA16_WGRAD", "0") != "0" or autograd_ops.MFMA16_WGRAD == 0
    monkeypatch.setattr(autograd_ops, "MFMA16_WGRAD", 0)
    shapes = [(b, h, w, ci, co, k, s) for b in (1, 2, 8) for h, w in ((240, 320), (60, 80), (15, 20))
              for ci, co in ((64, 64), (256, 128), (8, 8)) for k, s in ((3, 1), (3, 2), (1, 1))]
    assert not any(autograd_ops._wgrad16_selects(*sh, None) for sh in shapes)
    monkeypatch.setattr(autograd_ops, "MFMA16_WGRAD", 2)
    assert all(autograd_ops._wgrad16_selects(*sh, None) for sh in shapes)
    assert not autograd_ops._wgrad16_selects(2, 60, 80, 64, 64, 3, 1, (1, 1, 1, 1))       # explicit pads keep their path
    assert not autograd_ops._wgrad16_selects(2, 60, 80, 12, 16, 3, 1, None)
    assert not autograd_ops._wgrad16_selects(0, 60, 80, 64, 64, 3, 1, None)
    monkeypatch.setattr(autograd_ops, "MFMA16_WGRAD", 1)
    lib = _lib.lib()
    for sh in shapes:
        assert autograd_ops._wgrad16_selects(*sh, None) == bool(lib.sr_conv16_wgrad_prefers(*sh))


def _switches():
    return (autograd_ops.HALF_IO, autograd_ops.MFMA16, autograd_ops.STORE_HALF, autograd_ops.MFMA16_WGRAD)


def test_context_manager_sets_and_restores_the_four_switches(monkeypatch):
    monkeypatch.setattr(autograd_ops, "HALF_IO", False)
    monkeypatch.setattr(autograd_ops, "STORE_HALF", False)
    monkeypatch.setattr(autograd_ops, "MFMA16", 0)
    monkeypatch.setattr(autograd_ops, "MFMA16_WGRAD", 0)
    with experimental.autocast_mfma16():
        assert _switches() == (True, 1, True, 0)                        # wgrad defaults to 0: what the block did before
        with experimental.autocast_mfma16(mode=2, storage=False, wgrad=2):
            assert _switches() == (True, 2, True, 2)
        assert _switches() == (True, 1, True, 0)
        with experimental.autocast_mfma16(wgrad=1):
            assert _switches() == (True, 1, True, 1)
    assert _switches() == (False, 0, False, 0)
    with pytest.raises(RuntimeError):
        with experimental.autocast_mfma16(mode=2, storage=False, wgrad=2):
            assert _switches() == (True, 2, False, 2)
            raise RuntimeError("leave through an exception")
    assert _switches() == (False, 0, False, 0)
    for bad in (3, -1, "2", None):
        with pytest.raises(ValueError):
            with experimental.autocast_mfma16(wgrad=bad):
                pass
        assert _switches() == (False, 0, False, 0)
