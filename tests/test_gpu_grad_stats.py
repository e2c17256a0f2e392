"""Gradient statistics, clipping and the loss scaler of the optimiser step on the GPU (simplerecon_amd.optim: AdamW's
max_grad_norm / grad_stats, LossScaler, clip_grad_norm_; csrc/sr_optim.hip: sr_grad_stats, sr_adamw_step_clipped,
sr_grad_scale_inplace).

Bounds.  Norms: 1 ulp (fp32) of the float64 reference rounded to fp32 -- the double sum of N < 2^27 non-negative terms is
accurate to N * 2^-53 < 2^-26 relatively, far below half an fp32 ulp; sqrt, the division by the scale and one rounding add
at most one ulp.  Clip coefficient: 2.5 * 2^-23 relatively (1 ulp from the norm, half an ulp each for the rounded max_norm,
the addition and the division).  Clipped step: test_gpu_optim.py's bound, max |hip - f64| <= max(2 max |fp32 - f64|, 1 ulp
of the largest magnitude), against torch.optim.AdamW(foreach=False) on gradients multiplied by the coefficient the device
computed."""
import functools

import numpy as np
import pytest
import torch

from hostile_memory import bits
from simplerecon_amd import depth_model as dm
from simplerecon_amd import optim, synthetic, training

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALIGNED = [1, 3, 4, 5, 1023, 1025, 4097, optim.CHUNK + 1, 70000]   # every head, tail and chunk boundary
MISALIGNED = [1, 5, 1025]                                         # gradients one float past a 16-byte boundary: single floats
SIZES = ALIGNED + MISALIGNED
GROUPS = (dict(lr=1e-4, weight_decay=1e-4), dict(lr=1e-3, weight_decay=0.0))
SPLIT = 5            # tensors [0, SPLIT) are group 0, the others group 1
LATE, NEVER = 2, 6   # no gradient in the first two steps / in any step
STEPS = 10
MAX_NORM = 1.0       # far below the case's norm (about 2.6e3): every step clips
COEF_REL = 2.5 * 2.0 ** -23


@functools.lru_cache(maxsize=None)
def _case(seed=0, steps=STEPS):
    """(parameters, per-step gradients) on the CPU in fp32: per-tensor magnitudes 1e-6 .. 10, 5 % exact zeros."""
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=g) for n in SIZES]
    mags = [10.0 ** float(torch.rand((), generator=g) * 7 - 6) for _ in SIZES]
    mags[0], mags[len(ALIGNED) - 1] = 1e-6, 10.0
    grads = []
    for s in range(steps):
        row = []
        for i, n in enumerate(SIZES):
            if i == NEVER or (i == LATE and s < 2):
                row.append(None)
                continue
            x = torch.randn(n, generator=g) * mags[i]
            x[torch.rand(n, generator=g) < 0.05] = 0.0
            row.append(x)
        grads.append(row)
    return params, grads


def _grouped(ps, groups=GROUPS):
    return [dict(params=ps[:SPLIT], **groups[0]), dict(params=ps[SPLIT:], **groups[1])]


def _device_grad(gr, i, scale=1.0):
    """`gr * scale` on the device; for the MISALIGNED tensors a view that starts one float into a larger buffer."""
    x = (gr * scale).to(DEV)
    if i < len(ALIGNED):
        return x
    buf = torch.full((gr.numel() + 8,), -7.5, device=DEV)
    buf[1:1 + gr.numel()] = x
    view = buf[1:1 + gr.numel()]
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _assign(ps, row, scale=1.0):
    for i, (p, gr) in enumerate(zip(ps, row)):
        p.grad = None if gr is None else _device_grad(gr, i, scale)


def _snapshot(opt):
    """The statistics of the step just issued (device copies, no synchronisation)."""
    return {"norm": opt.grad_norm.clone(), "norms": opt.grad_norms.clone(), "coef": opt.clip_coef.clone(),
            "found_inf": opt.found_inf_last.clone()}


def _hip_run(params, grads, scaler=None, scale=1.0, snapshots=None, clip_first=None, **options):
    """`scale`: a number, or a function of the step index (the scale in force).  clip_first: optim.clip_grad_norm_ with
    that max_norm in front of every step."""
    ps = [p.clone().to(DEV).requires_grad_() for p in params]
    opt = optim.AdamW(_grouped(ps), **options)
    for s, row in enumerate(grads):
        _assign(ps, row, scale(s) if callable(scale) else scale)
        if clip_first is not None:
            optim.clip_grad_norm_(ps, clip_first)
        if scaler is not None:
            scaler.step(opt)
            scaler.update()
        else:
            opt.step()
        if snapshots is not None:
            snapshots.append(_snapshot(opt))
    torch.cuda.synchronize()
    return ps, opt


@functools.lru_cache(maxsize=None)
def _plain(steps):
    params, grads = _case()
    return _hip_run(params, grads[:steps])


@functools.lru_cache(maxsize=None)
def _clipped(steps=STEPS):
    """Case 3's run: `steps` fused clipped steps, with the statistics of every step.  Computed once, never written to."""
    params, grads = _case()
    snaps = []
    ps, opt = _hip_run(params, grads[:steps], snapshots=snaps, max_grad_norm=MAX_NORM)
    return ps, opt, snaps


def _oracle_run(params, grads, coefs, dtype):
    """torch.optim.AdamW(foreach=False) on the CPU after g.mul_(coef), step by step."""
    ps = [p.clone().to(dtype).requires_grad_() for p in params]
    opt = torch.optim.AdamW(_grouped(ps), foreach=False)
    for row, coef in zip(grads, coefs):
        for p, gr in zip(ps, row):
            p.grad = None if gr is None else gr.clone().to(dtype).mul_(coef)
        opt.step()
    return ps, opt


def _state(opt, p, key):
    s = opt.state.get(p)
    return s[key].detach() if s and key in s else torch.zeros_like(p.detach())


def _within_bound(what, hip, a, b):
    hip, a, b = hip.detach().cpu().double(), a.detach().cpu().double(), b.detach().cpu().double()
    err, base = float((hip - b).abs().max()), float((a - b).abs().max())
    ulp = float(np.spacing(np.float32(float(b.abs().max()))))
    bound = max(2.0 * base, ulp)
    print(f"{what}: |hip - f64| {err:.3e}, |fp32 - f64| {base:.3e}, ulp {ulp:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e} = max(2 x {base:.3e}, {ulp:.3e})"


def _check_against_oracle(hip_ps, hip_opt, refs, tag=""):
    (a_ps, a_opt), (b_ps, b_opt) = refs
    for i, (hp, ap, bp) in enumerate(zip(hip_ps, a_ps, b_ps)):
        name = f"{tag}tensor{i}[{hp.numel()}]"
        _within_bound(f"{name}.p", hp, ap, bp)
        for key in ("exp_avg", "exp_avg_sq"):
            _within_bound(f"{name}.{key}", _state(hip_opt, hp, key), _state(a_opt, ap, key), _state(b_opt, bp, key))


def _steps_of(sd, n):
    return [float(sd["state"][i]["step"]) if i in sd["state"] else None for i in range(n)]


def _same_bits(x, y):
    return x.shape == y.shape and bool((bits(x.detach()) == bits(y.detach())).all())


def _same_run(ps, opt, qs, opt2):
    for p, q in zip(ps, qs):
        assert _same_bits(p, q)
        for key in ("exp_avg", "exp_avg_sq", "step"):
            assert _same_bits(opt.state[p][key], opt2.state[q][key]), key


def _within_ulp(what, got, want64):
    """|got - fp32(want64)| <= 1 ulp of fp32(want64), elementwise."""
    got = np.asarray(got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got, dtype=np.float32).reshape(-1)
    with np.errstate(over="ignore"):
        want = np.asarray(want64, dtype=np.float64).reshape(-1).astype(np.float32)
    assert got.shape == want.shape and bool(np.isfinite(want).all()), what
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    ulp = np.spacing(np.abs(want)).astype(np.float64)
    worst = int(np.argmax(err / ulp))
    print(f"{what}: worst {err[worst] / ulp[worst]:.2f} ulp at {worst} ({got[worst]!r} against {want[worst]!r})")
    assert bool((err <= ulp).all()), f"{what}: {got[worst]!r} against {want[worst]!r} at {worst}"


def _stats_of(row, scaler=None, **options):
    """One step on `row`; the statistics and the parameters whose gradients it ran on."""
    params, _ = _case()
    ps = [p.clone().to(DEV).requires_grad_() for p in params]
    opt = optim.AdamW(_grouped(ps), **options)
    _assign(ps, row)
    if scaler is not None:
        scaler.step(opt)
        scaler.update()
    else:
        opt.step()
    torch.cuda.synchronize()
    return _snapshot(opt), ps


def _torch_scaler(**kw):
    """GradScaler with its device state in place (scaler.scale() creates it; these tests scale by hand)."""
    scaler = torch.amp.GradScaler("cuda", **kw)
    scaler.scale(torch.zeros((), device=DEV))
    return scaler


# ---- 1: norms -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("step", [0, 2])
def test_norms_are_within_one_ulp_of_float64(step):
    _, grads = _case()
    row = grads[step]
    got, ps = _stats_of(row, grad_stats=True)
    norms, total, found_inf, coef = optim.grad_stats_reference(row)
    _within_ulp("per-tensor norms", got["norms"], norms)
    _within_ulp("total norm", got["norm"], total)
    assert got["norms"].shape == (len(SIZES),) and got["norm"].dim() == 0 and got["norms"].dtype == torch.float32
    assert float(got["found_inf"]) == found_inf == 0.0 and float(got["coef"]) == coef == 1.0
    for i, gr in enumerate(row):
        assert (float(got["norms"][i]) == 0.0) == (gr is None or not bool(gr.any())), i
        if gr is not None:
            assert _same_bits(ps[i].grad.cpu(), gr)              # only read


def test_norms_of_gradients_whose_squares_leave_the_fp32_range():
    _, grads = _case()
    row = list(grads[2])
    g = torch.Generator().manual_seed(5)
    big, small = ALIGNED.index(1025), ALIGNED.index(1023)
    row[big] = torch.where(torch.rand(1025, generator=g) < 0.5, -1.0, 1.0) * 1e30
    row[small] = torch.where(torch.rand(1023, generator=g) < 0.5, -1.0, 1.0) * 1e-30
    mis = len(ALIGNED) + 2
    row[mis] = torch.where(torch.rand(1025, generator=g) < 0.5, -1.0, 1.0) * 1e-30      # and on the single-float path
    got, _ = _stats_of(row, grad_stats=True)
    norms, total, found_inf, _ = optim.grad_stats_reference(row)
    assert found_inf == 0.0 and float(got["found_inf"]) == 0.0           # (an fp32 accumulator overflows to inf here)
    assert norms[big] > 1e31 and 0.0 < norms[small] < 1e-28 and 0.0 < norms[mis] < 1e-28
    _within_ulp("per-tensor norms", got["norms"], norms)
    _within_ulp("total norm", got["norm"], total)


@pytest.mark.parametrize("which", ["torch", "hip"])
def test_norms_under_a_scaler_are_those_of_the_unscaled_gradients(which):
    _, grads = _case()
    plain, _ = _stats_of(grads[2], max_grad_norm=MAX_NORM)
    scaler = _torch_scaler(init_scale=2.0 ** 10) if which == "torch" else optim.LossScaler(init_scale=2.0 ** 10)
    scaled_row = [None if gr is None else gr * 2.0 ** 10 for gr in grads[2]]
    got, ps = _stats_of(scaled_row, scaler=scaler, max_grad_norm=MAX_NORM)
    for key in ("norm", "norms", "coef", "found_inf"):
        assert _same_bits(got[key], plain[key]), key
    assert float(plain["coef"]) < 1.0 and scaler.get_scale() == 2.0 ** 10
    for p, gr in zip(ps, scaled_row):
        if gr is not None:
            assert _same_bits(p.grad.cpu(), gr)                  # still scaled: nothing writes a gradient


# ---- 2: clip coefficient ---------------------------------------------------------------------------------------------------------

def test_clip_coefficient():
    _, grads = _case()
    _, _, snaps = _clipped()
    for s, snap in enumerate(snaps):
        _, total, _, coef = optim.grad_stats_reference(grads[s], max_norm=MAX_NORM)
        got = float(snap["coef"])
        print(f"step {s}: coefficient {got!r} against {coef!r}, relative error {abs(got - coef) / coef:.3e}")
        assert coef < 1.0 and abs(got - coef) <= COEF_REL * coef, s
        _within_ulp(f"step {s} total norm", snap["norm"], total)
    row = grads[2]
    _, total, _, _ = optim.grad_stats_reference(row)
    got, _ = _stats_of(row, max_grad_norm=2.0 * total)          # the norm is below max_norm: exactly 1
    assert float(got["coef"]) == 1.0 and bits(got["coef"]).item() == bits(torch.ones(())).item()


# ---- 3: clipped step ---------------------------------------------------------------------------------------------------------------

def test_clipped_step_parity_with_torch():
    params, grads = _case()
    ps, opt, snaps = _clipped()
    coefs = [float(snap["coef"]) for snap in snaps]
    assert len(coefs) == STEPS and all(0.0 < c < 1.0 for c in coefs)
    refs = tuple(_oracle_run(params, grads, coefs, dt) for dt in (torch.float32, torch.float64))
    _check_against_oracle(ps, opt, refs)
    want = _steps_of(refs[0][1].state_dict(), len(SIZES))
    assert want[LATE] == STEPS - 2 and want[NEVER] is None and want[0] == STEPS
    assert _steps_of(opt.state_dict(), len(SIZES)) == want
    assert not _same_bits(ps[0], _plain(STEPS)[0][0])            # (the clip did something)


# ---- 4: exactness --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("options", [dict(max_grad_norm=1e30), dict(grad_stats=True)], ids=["max_grad_norm_1e30", "grad_stats"])
def test_a_coefficient_of_one_changes_no_bit(options):
    params, grads = _case()
    snaps = []
    ps, opt = _hip_run(params, grads, snapshots=snaps, **options)
    _same_run(ps, opt, *_plain(STEPS))
    assert all(float(s["coef"]) == 1.0 and float(s["found_inf"]) == 0.0 for s in snaps)
    assert _steps_of(opt.state_dict(), len(SIZES)) == _steps_of(_plain(STEPS)[1].state_dict(), len(SIZES))


def test_fused_steps_leave_the_gradients_as_they_are():
    _, grads = _case()
    ps, _, _ = _clipped()
    for p, gr in zip(ps, grads[STEPS - 1]):
        assert (p.grad is None) == (gr is None)
        if gr is not None:
            assert _same_bits(p.grad.cpu(), gr)


def test_clip_grad_norm_then_a_plain_step_equals_the_fused_step():
    params, grads = _case()
    ps, opt = _hip_run(params, grads[:3], clip_first=MAX_NORM)
    qs, opt2, snaps = _clipped(3)
    _same_run(ps, opt, qs, opt2)
    # the free function wrote the gradients and returned the norm of what it found
    _assign(ps, grads[2])
    total = optim.clip_grad_norm_(ps, MAX_NORM)
    assert total.dim() == 0 and total.is_cuda and _same_bits(total, snaps[2]["norm"])
    coef = float(snaps[2]["coef"])
    for p, gr in zip(ps, grads[2]):
        if gr is not None:
            assert _same_bits(p.grad.cpu(), gr * coef)
    again = optim.clip_grad_norm_(ps, 1e30)                      # below max_norm: multiplied by exactly 1
    _within_ulp("norm of the clipped gradients", again, optim.grad_stats_reference([p.grad for p in ps])[1])
    for p, gr in zip(ps, grads[2]):
        if gr is not None:
            assert _same_bits(p.grad.cpu(), gr * coef)


# ---- 5: non-finite gradients -----------------------------------------------------------------------------------------------------------

BAD = {"inf_odd_tail": (ALIGNED.index(1025), 1024, float("inf")),
       "nan_first": (0, 0, float("nan")),
       "neg_inf_second_chunk": (ALIGNED.index(70000), optim.CHUNK + 5, float("-inf")),
       "inf_misaligned": (len(ALIGNED) + 2, 1023, float("inf"))}


@pytest.mark.parametrize("bad", list(BAD))
def test_non_finite_gradients_skip_the_step_and_back_off(bad):
    params, grads = _case()
    row = [None if gr is None else gr.clone() for gr in grads[2]]    # (step 2: every tensor but NEVER has a gradient)
    t, i, value = BAD[bad]
    row[t][i] = value
    scaler = optim.LossScaler(init_scale=2.0 ** 10)
    ps = [p.clone().to(DEV).requires_grad_() for p in params]
    opt = optim.AdamW(_grouped(ps), max_grad_norm=MAX_NORM)
    _assign(ps, row, 2.0 ** 10)
    scaler.step(opt)
    scaler.update()
    torch.cuda.synchronize()
    assert float(opt.found_inf_last) == 1.0 and optim.grad_stats_reference(row)[2] == 1.0
    assert scaler.get_scale() == 2.0 ** 9 and scaler._get_growth_tracker() == 0
    plan = opt._plan
    assert not bool(plan["exp_avg"].any()) and not bool(plan["exp_avg_sq"].any()) and not bool(plan["steps"].any())
    assert all(_same_bits(p.cpu(), p0) for p, p0 in zip(ps, params))
    assert opt.state_dict()["state"] == {}
    # the following finite step is step 1
    _assign(ps, grads[2], 2.0 ** 9)
    scaler.step(opt)
    scaler.update()
    torch.cuda.synchronize()
    assert float(opt.found_inf_last) == 0.0 and scaler.get_scale() == 2.0 ** 9 and scaler._get_growth_tracker() == 1
    coef = float(opt.clip_coef)
    refs = tuple(_oracle_run(params, [grads[2]], [coef], dt) for dt in (torch.float32, torch.float64))
    _check_against_oracle(ps, opt, refs)
    assert _steps_of(opt.state_dict(), len(SIZES)) == _steps_of(refs[0][1].state_dict(), len(SIZES))


# ---- 6: the scaler's rule ------------------------------------------------------------------------------------------------------------------

def test_scaler_rule_equals_torch_grad_scaler():
    ok, inf = torch.tensor([0.5, -1.0, 2.0, 0.0, 1.0]), torch.tensor([0.5, -1.0, float("inf"), 0.0, 1.0])
    kw = dict(init_scale=2.0 ** 10, growth_interval=2)

    def drive(ours, theirs, sequence):
        p, q = (torch.zeros(5, device=DEV).requires_grad_() for _ in range(2))
        opt_ours, opt_theirs = optim.AdamW([p]), optim.AdamW([q])
        for k, g in enumerate(sequence):
            p.grad, q.grad = g.to(DEV) * ours.get_scale(), g.to(DEV) * theirs.get_scale()
            ours.step(opt_ours)
            ours.update()
            ours.update()                       # a second update without a step: harmless
            theirs.step(opt_theirs)
            theirs.update()
            assert ours.get_scale() == theirs.get_scale(), k
            assert ours._get_growth_tracker() == int(theirs._growth_tracker), k
            assert float(opt_ours.found_inf_last) == float(bool(torch.isinf(g).any())), k
            assert _same_bits(p, q), k
    ours, theirs = optim.LossScaler(**kw), _torch_scaler(**kw)
    drive(ours, theirs, [ok, ok, inf, ok, ok, ok, inf, inf, ok])
    assert ours.get_scale() == 2.0 ** 9 and ours._get_growth_tracker() == 1       # x2, /2, x2, /2, /2 and one good step
    assert ours.state_dict() == theirs.state_dict()
    # each state dict loads into the other class, which continues equally
    ours2, theirs2 = optim.LossScaler(), torch.amp.GradScaler("cuda")
    ours2.load_state_dict(theirs.state_dict())
    theirs2.load_state_dict(ours.state_dict())
    theirs2.scale(torch.zeros((), device=DEV))
    assert ours2.state_dict() == theirs2.state_dict() == ours.state_dict()
    drive(ours2, theirs2, [ok, inf, ok, ok])
    drive(ours, theirs, [ok, inf, ok, ok])
    assert ours2.state_dict() == theirs2.state_dict() == ours.state_dict() == theirs.state_dict()
    # one optimiser per iteration, and only optim.AdamW
    p = torch.zeros(5, device=DEV).requires_grad_()
    p.grad = ok.to(DEV)
    opt = optim.AdamW([p])
    ours.step(opt)
    with pytest.raises(RuntimeError, match="already been called"):
        ours.step(opt)
    ours.update()
    with pytest.raises(TypeError):
        ours.step(torch.optim.AdamW([p]))


# ---- 7: the scale of this step ----------------------------------------------------------------------------------------------------------------

def test_the_step_divides_by_the_scale_its_loss_was_multiplied_by():
    params, grads = _case()
    scaler = optim.LossScaler(init_scale=2.0 ** 4, growth_interval=1)     # doubles after every finite step
    ps, opt = _hip_run(params, grads[:6], scaler=scaler, scale=lambda s: 2.0 ** (4 + s))
    assert scaler.get_scale() == 2.0 ** 10
    _same_run(ps, opt, *_plain(6))


# ---- 8: no synchronisation, no allocation -----------------------------------------------------------------------------------------------------------

def test_clipped_scaled_step_and_clip_grad_norm_do_not_synchronise():
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available")
    params, grads = _case()
    ps = [p.clone().to(DEV).requires_grad_() for p in params]
    dev_grads = [[None if gr is None else _device_grad(gr, i) for i, gr in enumerate(row)] for row in grads[2:7]]
    opt = optim.AdamW(_grouped(ps), max_grad_norm=MAX_NORM)
    scaler = optim.LossScaler(init_scale=1.0)
    loss = torch.ones((), device=DEV)

    def assign(row):
        for p, gr in zip(ps, row):
            p.grad = gr
    assign(dev_grads[0])
    scaler.scale(loss)
    scaler.step(opt)                # the first calls build the tables and the scaler's state
    scaler.update()
    optim.clip_grad_norm_(ps, 1e30)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        assign(dev_grads[1])
        allocations = torch.cuda.memory_stats()["allocation.all.allocated"]
        opt.step()
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == allocations      # no device allocation either
        assign(dev_grads[2])
        scaler.scale(loss)
        allocations = torch.cuda.memory_stats()["allocation.all.allocated"]
        scaler.step(opt)
        scaler.update()
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == allocations
        assign(dev_grads[3])
        total = optim.clip_grad_norm_(ps, 1e30)
        norm, norms = opt.grad_norm, opt.grad_norms              # reading them does not synchronise either
        opt.zero_grad()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert _steps_of(opt.state_dict(), len(SIZES))[0] == 3 and scaler.get_scale() == 1.0
    assert bool(torch.isfinite(total)) and float(total) > 0.0 and float(norm) > 0.0 and norms.shape == (len(SIZES),)


# ---- 9: determinism ------------------------------------------------------------------------------------------------------------------------------

def test_two_clipped_runs_are_bitwise_equal():
    params, grads = _case()
    snaps = []
    ps, opt = _hip_run(params, grads, snapshots=snaps, max_grad_norm=MAX_NORM)
    qs, opt2, snaps2 = _clipped()
    _same_run(ps, opt, qs, opt2)
    for a, b in zip(snaps, snaps2):
        for key in ("norm", "norms", "coef", "found_inf"):
            assert _same_bits(a[key], b[key]), key


# ---- 10: memory outside the operands ----------------------------------------------------------------------------------------------------------------

def test_statistics_read_no_memory_outside_their_operands():
    from test_gpu_uninitialised_memory import check_pipeline
    params, grads = _case()

    def make():
        scaler = optim.LossScaler(init_scale=2.0 ** 10)
        snaps = []
        ps, opt = _hip_run(params, grads[:3], scaler=scaler, scale=2.0 ** 10, snapshots=snaps, max_grad_norm=MAX_NORM)
        return {"p": [p.detach().clone() for p in ps],
                "exp_avg": [opt.state[p]["exp_avg"].clone() for p in ps],
                "exp_avg_sq": [opt.state[p]["exp_avg_sq"].clone() for p in ps],
                "steps": opt._plan["steps"].clone(),
                "norms": [s["norms"] for s in snaps], "norm": [s["norm"] for s in snaps],
                "coef": [s["coef"] for s in snaps], "found_inf": [s["found_inf"] for s in snaps],
                "scale": scaler._scale.clone(), "tracker": scaler._growth_tracker.clone()}
    check_pipeline(make, "clipped, scaled AdamW step")


# ---- 11: whole model ------------------------------------------------------------------------------------------------------------------------------------

def _training_model(B=2, K=3, h=32, w=48, **options):
    opts = dm.default_options(image_width=2 * w, image_height=2 * h, model_num_views=K + 1, matching_num_depth_bins=8, **options)
    model = dm.DepthModel(opts)
    for i, m in enumerate((model.encoder, model.matching_model, model.cost_volume_net, model.depth_decoder,
                           model.cost_volume.mlp)):
        synthetic.seeded_fill_(m, seed=11 + i)
    model = model.to(DEV).train()
    model.prior_on_side_stream = False
    return model, synthetic.training_batch(B, K, h, w, seed=6, device=DEV)


def test_whole_model_fp16_training_with_loss_scaler_and_clipping():
    model, batch = _training_model(clip_grad_norm=1.0)
    cfg = model.configure_optimizers()
    opt, sched = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
    assert isinstance(opt, optim.AdamW) and opt.max_grad_norm == 1.0
    scaler = optim.LossScaler(init_scale=2.0 ** 10)
    torch.manual_seed(0)
    losses = [training.train_step(model, batch, opt, sched, scaler, autocast_dtype=torch.float16, mfma16=2) for _ in range(3)]
    torch.cuda.synchronize()
    assert all(l.dim() == 0 and bool(torch.isfinite(l)) for l in losses)
    assert scaler.get_scale() == 2.0 ** 10 and float(opt.found_inf_last) == 0.0       # a skipped step would have halved it
    total = float(opt.grad_norm)
    assert np.isfinite(total) and total > 0.0
    params = list(model.parameters())
    norms = opt.grad_norms.cpu()
    assert norms.shape == (len(params),) and len(params) > 700
    with_grad = sum(p.grad is not None for p in params)
    assert with_grad > 100
    for i, p in enumerate(params):
        if p.grad is None:
            assert float(norms[i]) == 0.0, i
    assert int((norms > 0).sum()) > 100
    ref_norms, ref_total, found_inf, ref_coef = optim.grad_stats_reference([p.grad for p in params], scale=2.0 ** 10, max_norm=1.0)
    assert found_inf == 0.0
    _within_ulp("whole-model total norm", opt.grad_norm, ref_total)
    _within_ulp("whole-model per-tensor norms", norms, ref_norms)
    assert abs(float(opt.clip_coef) - ref_coef) <= COEF_REL * ref_coef
    assert max(float(s["step"]) for s in opt.state_dict()["state"].values()) == 3
    assert all(bool(torch.isfinite(p).all()) for p in params)
