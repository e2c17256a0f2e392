"""The HIP optimiser step (simplerecon_amd.optim.AdamW, csrc/sr_optim.hip) and the training loop around it
(simplerecon_amd.training) on the GPU.

Parity bound (cases 1, 9, 11), per tensor and for each of p, exp_avg and exp_avg_sq: with (a) torch.optim.AdamW(foreach=False) on
the CPU in fp32 and (b) the same in float64, max |hip - b| <= max(2 max |a - b|, 1 ulp of the tensor's largest magnitude).  Both
sides perform the same handful of roundings per element and step; only fused multiply-adds and evaluation order may differ.
Absolute, not relative: exp_avg cancels to near zero, where torch's own fp32 run is 1e-3 off float64 relatively.

The measured ratios error / bound of case 1 are written to $SR_ADAMW_PARITY_OUT (json) when that variable is set
(profiles/adamw_parity.json)."""
import copy
import functools
import json
import os

import numpy as np
import pytest
import torch

from hostile_memory import bits
from simplerecon_amd import depth_model as dm
from simplerecon_amd import ops, optim, synthetic, training

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [1, 3, 4, 5, 1023, 1025, 4097, optim.CHUNK + 1, 70000]   # every head, tail and chunk boundary
GROUPS = (dict(lr=1e-4, weight_decay=1e-4), dict(lr=1e-3, weight_decay=0.0))
SPLIT = 5            # tensors [0, SPLIT) are group 0, the others group 1
LATE, NEVER = 2, 6   # no gradient in the first two steps / in any step
STEPS = 10


@functools.lru_cache(maxsize=None)
def _case(seed=0, steps=STEPS):
    """(parameters, per-step gradients) on the CPU in fp32: per-tensor magnitudes 1e-6 .. 10, 5 % exact zeros."""
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(n, generator=g) for n in SIZES]
    mags = [10.0 ** float(torch.rand((), generator=g) * 7 - 6) for _ in SIZES]
    mags[0], mags[-1] = 1e-6, 10.0
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


def _oracle_run(params, grads, dtype, state_from=None):
    ps = [p.clone().to(dtype).requires_grad_() for p in params]
    opt = torch.optim.AdamW(_grouped(ps), foreach=False)
    if state_from is not None:
        opt.load_state_dict(state_from)
    for row in grads:
        for p, gr in zip(ps, row):
            p.grad = None if gr is None else gr.to(dtype)
        opt.step()
    return ps, opt


@functools.lru_cache(maxsize=None)
def _oracle(steps, dtype):
    """The reference after `steps` steps of _case(): computed once, shared, never written to."""
    params, grads = _case()
    return _oracle_run(params, grads[:steps], dtype)


def _hip_run(params, grads, groups=GROUPS, scaler=None, scale=1.0, state_from=None, sync=False):
    ps = [p.clone().to(DEV).requires_grad_() for p in params]
    opt = optim.AdamW(_grouped(ps, groups))
    if state_from is not None:
        opt.load_state_dict(state_from)
    for row in grads:
        for p, gr in zip(ps, row):
            p.grad = None if gr is None else (gr * scale).to(DEV)
        if scaler is not None:
            scaler.step(opt)
            scaler.update()
        else:
            opt.step()
        if sync:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    return ps, opt


@functools.lru_cache(maxsize=None)
def _hip(steps):
    params, grads = _case()
    return _hip_run(params, grads[:steps])


def _scaler():
    """GradScaler(init_scale=2^10) with its device state in place (scaler.scale() creates it; these tests scale by hand)."""
    scaler = torch.amp.GradScaler("cuda", init_scale=2.0 ** 10)
    scaler.scale(torch.zeros((), device=DEV))
    return scaler


def _state(opt, p, key):
    s = opt.state.get(p)
    return s[key].detach() if s and key in s else torch.zeros_like(p.detach())


def _within_bound(what, hip, a, b, ratios=None):
    hip, a, b = hip.detach().cpu().double(), a.detach().cpu().double(), b.detach().cpu().double()
    err, base = float((hip - b).abs().max()), float((a - b).abs().max())
    ulp = float(np.spacing(np.float32(float(b.abs().max()))))
    bound = max(2.0 * base, ulp)
    print(f"{what}: |hip - f64| {err:.3e}, |fp32 - f64| {base:.3e}, ulp {ulp:.3e}, bound {bound:.3e}, ratio {err / bound:.3f}")
    if ratios is not None:
        ratios[what] = {"error": err, "torch_fp32_error": base, "ulp": ulp, "ratio": err / bound}
    assert err <= bound, f"{what}: {err:.3e} > {bound:.3e} = max(2 x {base:.3e}, {ulp:.3e})"


def _check_against_oracle(hip_ps, hip_opt, steps_or_refs, ratios=None, tag=""):
    (a_ps, a_opt), (b_ps, b_opt) = steps_or_refs
    for i, (hp, ap, bp) in enumerate(zip(hip_ps, a_ps, b_ps)):
        name = f"{tag}tensor{i}[{hp.numel()}]"
        _within_bound(f"{name}.p", hp, ap, bp, ratios)
        for key in ("exp_avg", "exp_avg_sq"):
            _within_bound(f"{name}.{key}", _state(hip_opt, hp, key), _state(a_opt, ap, key), _state(b_opt, bp, key), ratios)


def _steps_of(sd, n):
    return [float(sd["state"][i]["step"]) if i in sd["state"] else None for i in range(n)]


def _same_bits(x, y):
    return x.shape == y.shape and bool((bits(x.detach()) == bits(y.detach())).all())


# ---- 1: parity ---------------------------------------------------------------------------------------------------------------

def test_parity_with_torch_adamw():
    ratios = {}
    hip_ps, hip_opt = _hip(STEPS)
    refs = (_oracle(STEPS, torch.float32), _oracle(STEPS, torch.float64))
    _check_against_oracle(hip_ps, hip_opt, refs, ratios)
    want = _steps_of(refs[0][1].state_dict(), len(SIZES))
    assert want[LATE] == STEPS - 2 and want[NEVER] is None and want[0] == STEPS
    assert _steps_of(hip_opt.state_dict(), len(SIZES)) == want
    out = os.environ.get("SR_ADAMW_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "steps": STEPS, "sizes": SIZES, "groups": GROUPS,
                       "bound": "max(2 x |torch fp32 - torch f64|, 1 ulp of the tensor's largest magnitude), against torch f64",
                       "worst_ratio": max(r["ratio"] for r in ratios.values()), "tensors": ratios}, f, indent=1)


# ---- 2: exact cases ------------------------------------------------------------------------------------------------------------

def test_zero_gradients_only_decay_the_parameters():
    params, _ = _case()
    zeros = [[torch.zeros_like(p) for p in params]]
    ps, opt = _hip_run(params, zeros)
    for i, (p, p0) in enumerate(zip(ps, params)):
        grp = GROUPS[0 if i < SPLIT else 1]
        want = p0.numpy() * np.float32(1.0 - grp["lr"] * grp["weight_decay"])
        assert want.dtype == np.float32 and np.array_equal(p.detach().cpu().numpy().view(np.int32), want.view(np.int32)), i
        assert not bool(opt.state[p]["exp_avg"].any()) and not bool(opt.state[p]["exp_avg_sq"].any())
    ps, _ = _hip_run(params, zeros, groups=(dict(lr=1e-4, weight_decay=0.0), dict(lr=1e-3, weight_decay=0.0)))
    assert all(_same_bits(p.cpu(), p0) for p, p0 in zip(ps, params))


# ---- 3: misaligned views -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 5, 1025])
def test_misaligned_views(n):
    g = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) for _ in range(3)]

    def run(offset):
        flat = torch.full((n + offset + 7,), 123.25, device=DEV)
        flat[offset:offset + n] = p0.to(DEV)
        gflat = torch.full((n + offset + 7,), -7.5, device=DEV)
        p = flat[offset:offset + n].requires_grad_()
        assert p.data_ptr() % 16 == 4 * offset and p.is_leaf
        opt = optim.AdamW([p], lr=1e-3, weight_decay=1e-2)
        for gr in grads:
            gflat[offset:offset + n] = gr.to(DEV)
            p.grad = gflat[offset:offset + n]
            opt.step()
        torch.cuda.synchronize()
        return flat, gflat, p, opt
    flat_a, _, p_a, opt_a = run(0)
    flat_m, gflat_m, p_m, opt_m = run(1)
    assert bool((p_a.detach().cpu() != p0).any())
    assert _same_bits(p_a, p_m)
    for key in ("exp_avg", "exp_avg_sq", "step"):
        assert _same_bits(opt_a.state[p_a][key], opt_m.state[p_m][key]), key
    for buf, fill in ((flat_m, 123.25), (gflat_m, -7.5), (flat_a, 123.25)):
        off = 1 if buf is not flat_a else 0
        outside = torch.cat([buf[:off], buf[off + n:]])
        assert _same_bits(outside, torch.full_like(outside, fill))
    assert _same_bits(gflat_m[1:1 + n].cpu(), grads[-1])


# ---- 4, 5: loss scaling ---------------------------------------------------------------------------------------------------------

def test_loss_scaling_is_exact_and_leaves_the_gradients():
    params, grads = _case()
    scaler = _scaler()
    ps, opt = _hip_run(params, grads, scaler=scaler, scale=2.0 ** 10)
    plain_ps, plain_opt = _hip(STEPS)
    assert scaler.get_scale() == 2.0 ** 10
    for p, q, gr in zip(ps, plain_ps, grads[-1]):
        assert _same_bits(p, q)
        for key in ("exp_avg", "exp_avg_sq", "step"):
            assert _same_bits(opt.state[p][key], plain_opt.state[q][key]), key
        if gr is not None:
            assert _same_bits(p.grad.cpu(), gr * 2.0 ** 10)     # still scaled: the kernel only reads gradients


@pytest.mark.parametrize("bad", ["inf_last", "nan_first"])
def test_non_finite_gradients_skip_the_whole_step(bad):
    params, grads = _case()
    row = [None if gr is None else gr.clone() for gr in grads[2]]    # (step 2: every tensor but NEVER has a gradient)
    if bad == "inf_last":
        row[-1][-1] = float("inf")
    else:
        row[0][0] = float("nan")
    scaler = _scaler()
    ps = [p.clone().to(DEV).requires_grad_() for p in params]
    opt = optim.AdamW(_grouped(ps))
    for p, gr in zip(ps, row):
        p.grad = None if gr is None else (gr * 2.0 ** 10).to(DEV)
    scaler.step(opt)
    scaler.update()
    torch.cuda.synchronize()
    assert scaler.get_scale() == 2.0 ** 9
    plan = opt._plan
    assert not bool(plan["exp_avg"].any()) and not bool(plan["exp_avg_sq"].any()) and not bool(plan["steps"].any())
    assert all(_same_bits(p.cpu(), p0) for p, p0 in zip(ps, params))
    assert opt.state_dict()["state"] == {}
    # the following finite step is step 1
    for p, gr in zip(ps, grads[2]):
        p.grad = None if gr is None else (gr * 2.0 ** 9).to(DEV)
    scaler.step(opt)
    scaler.update()
    torch.cuda.synchronize()
    assert scaler.get_scale() == 2.0 ** 9
    refs = tuple(_oracle_run(params, [grads[2]], dt) for dt in (torch.float32, torch.float64))
    _check_against_oracle(ps, opt, refs)
    assert _steps_of(opt.state_dict(), len(SIZES)) == _steps_of(refs[0][1].state_dict(), len(SIZES))
    plain_ps, _ = _hip_run(params, [grads[2]])
    assert all(_same_bits(p, q) for p, q in zip(ps, plain_ps))


# ---- 6: no host synchronisation ---------------------------------------------------------------------------------------------------

def test_step_does_not_synchronise_with_the_host():
    if not hasattr(torch.cuda, "set_sync_debug_mode"):
        pytest.skip("torch.cuda.set_sync_debug_mode is not available")
    params, grads = _case()
    ps = [p.clone().to(DEV).requires_grad_() for p in params]
    dev_grads = [[None if gr is None else gr.to(DEV) for gr in row] for row in grads[:4]]
    opt = optim.AdamW(_grouped(ps))
    scaler = _scaler()

    def assign(row):
        for p, gr in zip(ps, row):
            p.grad = gr
    assign(dev_grads[0])
    opt.step()                      # the first call builds the tables
    assign(dev_grads[1])
    scaler.step(opt)                # (and the scaler's first call its own state)
    scaler.update()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        assign(dev_grads[2])
        allocations = torch.cuda.memory_stats()["allocation.all.allocated"]
        opt.step()
        assert torch.cuda.memory_stats()["allocation.all.allocated"] == allocations      # no device allocation either
        assign(dev_grads[3])
        scaler.step(opt)            # (the scaler allocates its flags; it must not synchronise)
        scaler.update()
        opt.zero_grad()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert _steps_of(opt.state_dict(), len(SIZES))[0] == 4


# ---- 7: gradient addresses and the pointer ring ------------------------------------------------------------------------------------

def test_fresh_gradient_addresses_every_step_without_synchronising():
    params, grads = _case()
    queued = 2 * optim.RING_SLOTS + 3         # the ring wraps twice; the first three steps are the issue's case
    rows = [grads[s % STEPS] for s in range(queued)]
    dev_grads = [[None if gr is None else gr.to(DEV) for gr in row] for row in rows]    # all alive: all at their own addresses
    ps = [p.clone().to(DEV).requires_grad_() for p in params]
    opt = optim.AdamW(_grouped(ps))
    busy = torch.randn(4096, 4096, device=DEV)
    torch.cuda.synchronize()
    for _ in range(20):                      # the device falls behind the host, so that copies of the table are pending
        busy = torch.mm(busy, busy).clamp_(-1.0, 1.0)
    for s, row in enumerate(dev_grads):
        opt.zero_grad(set_to_none=s % 2 == 0)
        for p, gr in zip(ps, row):
            p.grad = gr.clone() if gr is not None and s % 2 else gr      # (a clone is one more new address)
        opt.step()
    torch.cuda.synchronize()
    want_ps, want_opt = _hip_run(params, rows, sync=True)
    for p, q in zip(ps, want_ps):
        assert _same_bits(p, q)
        for key in ("exp_avg", "exp_avg_sq", "step"):
            assert _same_bits(opt.state[p][key], want_opt.state[q][key]), key
    refs = tuple(_oracle_run(params, rows, dt) for dt in (torch.float32, torch.float64))
    _check_against_oracle(ps, opt, refs)


# ---- 8: determinism -----------------------------------------------------------------------------------------------------------------

def test_two_runs_are_bitwise_equal():
    params, grads = _case()
    ps, opt = _hip_run(params, grads)
    qs, opt2 = _hip(STEPS)
    for p, q in zip(ps, qs):
        assert _same_bits(p, q)
        for key in ("exp_avg", "exp_avg_sq", "step"):
            assert _same_bits(opt.state[p][key], opt2.state[q][key]), key


# ---- 9: checkpoints -----------------------------------------------------------------------------------------------------------------

def test_checkpoint_from_hip_to_torch_and_back():
    params, grads = _case()
    refs = (_oracle(5, torch.float32), _oracle(5, torch.float64))
    hip_ps, hip_opt = _hip_run(params, grads[:3])
    sd = hip_opt.state_dict()
    assert set(sd["param_groups"][0]) == set(torch.optim.AdamW([torch.zeros(1)]).state_dict()["param_groups"][0])
    assert all(set(s) == {"step", "exp_avg", "exp_avg_sq"} for s in sd["state"].values())
    # HIP -> torch: two more steps on each side
    cpu_ps, cpu_opt = _oracle_run([p.detach().cpu() for p in hip_ps], grads[3:5], torch.float32, state_from=copy.deepcopy(sd))
    _check_against_oracle(cpu_ps, cpu_opt, refs, tag="hip->torch ")
    for row in grads[3:5]:
        for p, gr in zip(hip_ps, row):
            p.grad = None if gr is None else gr.to(DEV)
        hip_opt.step()
    torch.cuda.synchronize()
    _check_against_oracle(hip_ps, hip_opt, refs, tag="hip ")
    assert _steps_of(cpu_opt.state_dict(), len(SIZES)) == _steps_of(hip_opt.state_dict(), len(SIZES))
    # torch -> HIP
    t_ps, t_opt = _oracle_run(params, grads[:3], torch.float32)
    h_ps, h_opt = _hip_run([p.detach() for p in t_ps], grads[3:5], state_from=copy.deepcopy(t_opt.state_dict()))
    _check_against_oracle(h_ps, h_opt, refs, tag="torch->hip ")
    assert _steps_of(h_opt.state_dict(), len(SIZES)) == _steps_of(refs[0][1].state_dict(), len(SIZES))


# ---- 10: memory outside the operands ---------------------------------------------------------------------------------------------------

def test_step_reads_no_memory_outside_its_operands():
    from test_gpu_uninitialised_memory import check_pipeline
    params, grads = _case()

    def make():
        scaler = _scaler()
        ps, opt = _hip_run(params, grads[:3], scaler=scaler, scale=2.0 ** 10)
        return {"p": [p.detach().clone() for p in ps],
                "exp_avg": [opt.state[p]["exp_avg"].clone() for p in ps],
                "exp_avg_sq": [opt.state[p]["exp_avg_sq"].clone() for p in ps],
                "steps": opt._plan["steps"].clone()}
    check_pipeline(make, "AdamW step")


# ---- 11: whole model -------------------------------------------------------------------------------------------------------------------

def _training_model(B=2, K=3, h=32, w=48):
    opts = dm.default_options(image_width=2 * w, image_height=2 * h, model_num_views=K + 1, matching_num_depth_bins=8)
    model = dm.DepthModel(opts)
    for i, m in enumerate((model.encoder, model.matching_model, model.cost_volume_net, model.depth_decoder,
                           model.cost_volume.mlp)):
        synthetic.seeded_fill_(m, seed=11 + i)
    model = model.to(DEV).train()
    model.prior_on_side_stream = False
    return model, synthetic.training_batch(B, K, h, w, seed=6, device=DEV)


def _eval_forward(model, batch):
    cur, src = batch
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            out = model.forward_tensors(cur["image_b3hw"], src["image_b3hw"],
                                        src["cam_T_world_b44"] @ cur["world_T_cam_b44"].unsqueeze(1),
                                        cur["cam_T_world_b44"].unsqueeze(1) @ src["world_T_cam_b44"],
                                        src["K_s1_b44"], cur["invK_s1_b44"])
        torch.cuda.synchronize()
        return out["depth_pred_s0_b1hw"].clone()
    finally:
        model.train(was_training)


def test_whole_model_step_reaches_the_packed_weights():
    model, batch = _training_model()
    torch.manual_seed(0)
    model.step("train", batch).backward()
    before = _eval_forward(model, batch)            # packs every weight from the parameters as they are
    named = list(model.named_parameters())
    assert len(named) > 700
    p0 = [p.detach().cpu().clone() for _, p in named]
    g0 = [None if p.grad is None else p.grad.detach().cpu().clone() for _, p in named]
    versions = [p._version for _, p in named]
    opt = optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    opt.step()
    torch.cuda.synchronize()
    # (i) version counters
    with_grad = sum(g is not None for g in g0)
    assert with_grad > 100
    for (name, p), v, g in zip(named, versions, g0):
        assert (p._version > v) if g is not None else (p._version == v), name
    # (ii) the next forward runs on the new weights
    after = _eval_forward(model, batch)
    fresh = copy.deepcopy(model)
    ops.forget_packed(fresh)
    want = _eval_forward(fresh, batch)
    assert bool(torch.isfinite(after).all())
    assert _same_bits(after, want), float((after - want).abs().max())
    assert not _same_bits(after, before)
    # (iii) parity of every parameter
    refs = []
    for dt in (torch.float32, torch.float64):
        ps = [p.clone().to(dt).requires_grad_() for p in p0]
        for p, g in zip(ps, g0):
            p.grad = None if g is None else g.to(dt)
        torch.optim.AdamW(ps, lr=1e-4, weight_decay=1e-4, foreach=False).step()
        refs.append(ps)
    worst = 0.0
    for (name, p), a, b in zip(named, *refs):
        hip, a, b = p.detach().cpu().double(), a.detach().double(), b.detach().double()
        err, base = float((hip - b).abs().max()), float((a - b).abs().max())
        bound = max(2.0 * base, float(np.spacing(np.float32(float(b.abs().max())))))
        worst = max(worst, err / bound)
        assert err <= bound, f"{name}: {err:.3e} > {bound:.3e}"
    print(f"whole model: {len(named)} tensors, {with_grad} with a gradient, worst error / bound {worst:.3f}")


# ---- 12: train_step and fit ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dt", [None, torch.float16], ids=["fp32", "fp16_mfma16"])
def test_train_step_and_fit(dt):
    model, batch = _training_model()
    cfg = model.configure_optimizers()
    opt, sched = cfg["optimizer"], cfg["lr_scheduler"]["scheduler"]
    assert isinstance(opt, optim.AdamW) and cfg["lr_scheduler"]["interval"] == "step"
    assert opt.param_groups[0]["lr"] == 1e-4 and opt.param_groups[0]["weight_decay"] == 1e-4
    scaler = _scaler() if dt is not None else None
    p0 = [p.detach().clone() for p in model.parameters()]
    torch.manual_seed(0)
    losses = [training.train_step(model, batch, opt, sched, scaler, autocast_dtype=dt, mfma16=2 if dt is not None else None)
              for _ in range(3)]
    torch.cuda.synchronize()
    assert all(l.dim() == 0 and not l.requires_grad and bool(torch.isfinite(l)) for l in losses)
    assert sched.last_epoch == 3
    with_grad = sum(p.grad is not None for p in model.parameters())
    changed = sum(not _same_bits(p, q) for p, q in zip(model.parameters(), p0))
    assert with_grad > 100 and changed > 0.9 * with_grad, (changed, with_grad)
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
    if scaler is not None:
        assert scaler.get_scale() == 2.0 ** 10                       # a skipped step would have halved it
    assert max(float(s["step"]) for s in opt.state_dict()["state"].values()) == 3
    if dt is None:
        def forever():
            while True:
                yield batch
        seen = []
        assert training.fit(model, forever(), 2, optimizer=opt, scheduler=sched, on_step=lambda s, l: seen.append(s)) == 2
        assert seen == [1, 2] and sched.last_epoch == 5
        assert training.fit(model, [batch], 5, optimizer=opt, scheduler=sched) == 1     # the iterable ended first
