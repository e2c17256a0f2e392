"""Host side of the gradient statistics (simplerecon_amd.optim: grad_stats_reference, LossScaler, clip_grad_norm_ and the
max_grad_norm / grad_stats options) and the argument rules of their C entry points.  Runs without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from simplerecon_amd import _lib, optim
from simplerecon_amd import depth_model as dm
from simplerecon_amd._lib import HipLibraryError

SIZES = [1, 3, 4, 5, 1023, 1025, 4097, optim.CHUNK + 1, 70000]
NEVER = 6
# Two float64 evaluations of the same sums of N < 2^17 non-negative terms differ by at most the worst case of a sequential sum,
# N * 2^-53 relatively, whatever order either side adds in (torch also takes the norm of the per-tensor norms).
REL = 2.0 ** 17 * 2.0 ** -53


def _grads(seed=0):
    """Per-tensor magnitudes 1e-6 .. 10, 5 % exact zeros, one tensor without a gradient."""
    g = torch.Generator().manual_seed(seed)
    mags = [10.0 ** float(torch.rand((), generator=g) * 7 - 6) for _ in SIZES]
    mags[0], mags[-1] = 1e-6, 10.0
    out = []
    for i, n in enumerate(SIZES):
        x = torch.randn(n, generator=g) * mags[i]
        x[torch.rand(n, generator=g) < 0.05] = 0.0
        out.append(None if i == NEVER else x)
    return out


@pytest.mark.parametrize("max_norm", [1.0, 1e-3, 1e6])
def test_reference_equals_torch_clip_grad_norm_in_float64(max_norm):
    grads = _grads()
    ps = [torch.zeros(n, dtype=torch.float64, requires_grad=True) for n in SIZES]
    for p, g in zip(ps, grads):
        p.grad = None if g is None else g.double()
    total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False))
    norms, ref_total, found_inf, coef = optim.grad_stats_reference(grads, max_norm=max_norm)
    assert found_inf == 0.0 and norms.shape == (len(SIZES),) and norms[NEVER] == 0.0
    assert abs(ref_total - total) <= REL * total
    for n, g in zip(norms, grads):
        if g is not None:
            want = float(torch.linalg.vector_norm(g.double()))
            assert abs(n - want) <= REL * want
    want_coef = min(1.0, max_norm / (total + 1e-6))
    assert abs(coef - want_coef) <= REL * want_coef and (coef == 1.0) == (max_norm == 1e6)
    for p, g in zip(ps, grads):                  # torch multiplied in place by the same coefficient
        if g is not None:
            assert torch.allclose(p.grad, g.double() * coef, rtol=REL, atol=0.0)


def test_reference_scale_flag_and_extreme_magnitudes():
    grads = _grads()
    norms, total, _, coef = optim.grad_stats_reference(grads, max_norm=1.0)
    scaled = [None if g is None else g * 1024.0 for g in grads]
    norms_s, total_s, found_inf, coef_s = optim.grad_stats_reference(scaled, scale=1024.0, max_norm=1.0)
    assert np.array_equal(norms, norms_s) and total == total_s and coef == coef_s and found_inf == 0.0
    assert optim.grad_stats_reference(grads)[3] == 1.0
    big, small = torch.full((1025,), 1e30), torch.full((1023,), -1e-30)     # squares outside the fp32 range
    norms, total, found_inf, _ = optim.grad_stats_reference([big, small])
    assert found_inf == 0.0 and abs(norms[0] - 1e30 * 1025 ** 0.5) <= 1e-6 * norms[0]
    assert abs(norms[1] - 1e-30 * 1023 ** 0.5) <= 1e-6 * norms[1] and abs(total - norms[0]) <= 1e-12 * total
    for bad in (float("inf"), float("-inf"), float("nan")):
        x = torch.ones(5)
        x[4] = bad
        assert optim.grad_stats_reference([torch.ones(3), x])[2] == 1.0


def test_loss_scaler_has_the_grad_scaler_schema_and_defaults():
    ours = optim.LossScaler()                    # no device state before the first scale() / step()
    theirs = torch.amp.GradScaler("cpu")
    assert theirs.is_enabled()
    assert ours.state_dict() == theirs.state_dict()
    assert list(ours.state_dict()) == ["scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"]
    assert ours.get_scale() == 65536.0 and ours.get_growth_factor() == 2.0 and ours.get_backoff_factor() == 0.5
    assert ours.get_growth_interval() == 2000
    theirs = torch.amp.GradScaler("cpu", init_scale=8.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=7)
    ours.load_state_dict(theirs.state_dict())
    assert ours.state_dict() == theirs.state_dict() and ours.get_scale() == 8.0
    back = torch.amp.GradScaler("cpu")
    back.load_state_dict(optim.LossScaler(init_scale=4.0, growth_interval=3).state_dict())
    assert back.state_dict() == optim.LossScaler(init_scale=4.0, growth_interval=3).state_dict()
    with pytest.raises(RuntimeError):
        ours.load_state_dict({})
    ours.update()
    ours.update(new_scale=2.0)                   # harmless without a step; a new scale is kept for the device state
    assert ours.get_scale() == 2.0


def test_loss_scaler_refusals():
    p = torch.zeros(4, requires_grad=True)
    scaler = optim.LossScaler()
    with pytest.raises(TypeError, match="optim.AdamW only"):
        scaler.step(torch.optim.AdamW([p]))
    with pytest.raises(TypeError):
        scaler.step(torch.optim.SGD([p], lr=0.1))
    with pytest.raises(HipLibraryError):
        scaler.scale(torch.zeros(()))            # a host tensor: no CPU fallback
    with pytest.raises(HipLibraryError):
        optim.LossScaler(device="cpu")
    with pytest.raises(ValueError):
        optim.LossScaler(growth_factor=1.0)
    with pytest.raises(ValueError):
        optim.LossScaler(backoff_factor=1.0)
    with pytest.raises(ValueError):
        optim.LossScaler(growth_interval=0)


def test_clip_options_and_free_function_refusals():
    p = torch.zeros(4, 6, requires_grad=True)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-50):      # (1e-50 is zero in fp32, which the kernel reads as "off")
        with pytest.raises(ValueError, match="max_norm"):
            optim.AdamW([p], max_grad_norm=bad)
        with pytest.raises(ValueError, match="max_norm"):
            optim.clip_grad_norm_([p], bad)
    with pytest.raises(HipLibraryError):         # the options change nothing about the refusal of host parameters
        optim.AdamW([p], max_grad_norm=1.0, grad_stats=True)
    with pytest.raises(NotImplementedError, match="L2"):
        optim.clip_grad_norm_([p], 1.0, norm_type=float("inf"))
    with pytest.raises(NotImplementedError):
        optim.clip_grad_norm_([p], 1.0, norm_type=1)
    assert float(optim.clip_grad_norm_([p], 1.0)) == 0.0           # no gradient anywhere: torch's answer
    p.grad = torch.zeros(4, 6)
    with pytest.raises(HipLibraryError):         # a good gradient, but on the host
        optim.clip_grad_norm_([p], 1.0)
    p.grad = torch.zeros(4, 6).to_sparse()
    with pytest.raises(RuntimeError, match="sparse"):
        optim.clip_grad_norm_([p], 1.0)
    q = torch.zeros(4, 6, dtype=torch.float16, requires_grad=True)
    q.grad = torch.zeros(4, 6, dtype=torch.float16)
    with pytest.raises(TypeError, match="contiguous float32"):
        optim.clip_grad_norm_([q], 1.0)


def test_clip_grad_norm_option_defaults_to_off():
    assert dm.default_options().clip_grad_norm == 0.0
    assert dm.default_options(clip_grad_norm=0.5).clip_grad_norm == 0.5


def test_entry_points_refuse_null_and_misaligned_tables():
    """Every refusal comes before the first launch: the addresses are never read, so this runs without a device."""
    lib = _lib.lib()
    INVALID, UNSUPPORTED, TOO_SMALL = 1, 2, 3
    A = 0x10000                                   # an aligned address nothing reads
    assert lib.sr_grad_stats_workspace_bytes(12, 3) >= 12 * 8 and lib.sr_grad_stats_workspace_bytes(0, 1) >= 8
    ws = lib.sr_grad_stats_workspace_bytes(12, 3)

    def stats(g=A, numel=A, cs=A, T=3, chunks=12, scale=None, max_norm=1.0, norms=A, out=A, s_scale=None, s_tracker=None,
              growth=2.0, backoff=0.5, interval=2000, work=A, bytes_=ws):
        return lib.sr_grad_stats(g, numel, cs, T, chunks, scale, max_norm, norms, out, s_scale, s_tracker, growth, backoff,
                                 interval, work, bytes_, None)
    for kw in (dict(g=None), dict(numel=None), dict(cs=None), dict(norms=None), dict(out=None), dict(work=None),
               dict(g=A + 4), dict(numel=A + 4), dict(cs=A + 2), dict(norms=A + 2), dict(out=A + 1), dict(work=A + 4),
               dict(scale=A + 2), dict(s_scale=A + 2, s_tracker=A), dict(s_scale=A, s_tracker=A + 2),
               dict(T=0), dict(chunks=-1), dict(max_norm=float("nan")),
               dict(s_scale=A), dict(s_tracker=A), dict(s_scale=A, s_tracker=A, scale=A),
               dict(s_scale=A, s_tracker=A, growth=0.0), dict(s_scale=A, s_tracker=A, backoff=float("nan")),
               dict(s_scale=A, s_tracker=A, interval=0)):
        assert stats(**kw) == INVALID, kw
    assert stats(T=(1 << 20) + 1) == UNSUPPORTED
    assert stats(bytes_=ws - 1) == TOO_SMALL

    def scale_inplace(g=A, numel=A, cs=A, T=3, chunks=12, coef=A):
        return lib.sr_grad_scale_inplace(g, numel, cs, T, chunks, coef, None)
    for kw in (dict(g=None), dict(numel=None), dict(cs=None), dict(coef=None), dict(g=A + 4), dict(numel=A + 4),
               dict(cs=A + 2), dict(coef=A + 2), dict(T=0), dict(chunks=-1)):
        assert scale_inplace(**kw) == INVALID, kw
    assert scale_inplace(T=(1 << 20) + 1) == UNSUPPORTED

    groups = (C.c_double * 5)(1e-3, 0.9, 0.999, 1e-8, 1e-2)

    def clipped(tables=(A,) * 9, coef=A, scale=None, found_inf=None):
        return lib.sr_adamw_step_clipped(*tables, 3, 12, C.addressof(groups), 1, scale, found_inf, coef, None)
    assert clipped(coef=A + 2) == INVALID and clipped(scale=A + 1) == INVALID
    for k in range(9):
        assert clipped(tables=tuple(None if i == k else A for i in range(9))) == INVALID, k
        assert clipped(tables=tuple(A + 2 if i == k else A for i in range(9))) == INVALID, k
