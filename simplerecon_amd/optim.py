"""The optimiser step of the training path: multi-tensor AdamW on the HIP kernels of csrc/sr_optim.hip
(include/simplerecon_hip.h, section "optimiser").

    opt = optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    loss.backward(); opt.step()                     # two launches for every parameter tensor of the model
    scaler.step(opt); scaler.update()               # torch.amp.GradScaler: unscale and skip inside the kernel, no host sync

A `torch.optim.Optimizer`: parameter groups, `zero_grad`, `add_param_group` and LR schedulers work unchanged, and
`state_dict()` / `load_state_dict()` use torch.optim.AdamW's schema (per-parameter `step`, `exp_avg`, `exp_avg_sq`), so a
checkpoint moves between the two classes in both directions.  The arithmetic is torch's `_single_tensor_adam` with
decoupled weight decay, one rounded fp32 operation per line (the header has the rule).

What differs from torch.optim.AdamW:
  * Gradients are only read.  Under a GradScaler torch's fused kernel writes the unscaled gradient back into `p.grad`; this
    one divides in registers and leaves `p.grad` as backward wrote it (still multiplied by the scale).
  * The kernels write parameters through raw pointers, which bumps no version counter, while every packed / folded weight
    (ops._cached, ops._state_key) and graph.GraphedCallable(check_weights=True) is keyed on `tensor._version`.  step()
    therefore bumps the counter of every parameter that had a gradient (torch.autograd.graph.increment_version) -- also
    on a step that `found_inf` turns into a no-op on the device: the host does not know about the skip, and packing an
    unchanged weight again is harmless.
  * State lives in one flat fp32 buffer for `exp_avg`, one for `exp_avg_sq` and one array of per-tensor step counts, all
    on the device; `self.state[p]` holds views into them.  A parameter that receives no gradient in a step is not
    touched and its step count does not advance (torch's rule).  state_dict() lists the parameters whose count is above
    zero, as torch lists those that ever had a gradient, and returns copies.
  * No fallback: amsgrad, maximize, differentiable, capturable, foreach / fused requests, sparse gradients, parameters or
    gradients that are not contiguous fp32 device tensors, and parameters on more than one device raise.

After the first call step() allocates nothing on the device and never synchronises with the host: gradient addresses
(new every step under zero_grad(set_to_none=True)) go to the device in one asynchronous copy from a ring of pinned
tables, each slot guarded by an event so that it is not rewritten while an earlier step's copy may be pending.

Out of scope: gradient clipping and norms, a loss scaler of our own (torch's inf check over the gradients stays),
writing packed or 16-bit weights from inside the kernel, HIP-graph capture of the step, 16-bit parameters and sharded
state."""
import ctypes as C

import numpy as np
import torch

from . import _lib

CHUNK = 4096        # SR_ADAMW_CHUNK: elements one workgroup updates
MAX_GROUPS = 16     # SR_ADAMW_MAX_GROUPS
RING_SLOTS = 8      # pinned gradient-address tables in flight
_ALIGN = 4          # state views start at multiples of 4 elements: 16-byte accesses whenever p and g allow them


def chunk_plan(numels, chunk=CHUNK):
    """Prefix table of the streaming launch: chunk_start[t] = number of chunks in front of tensor t, chunk_start[T] = the
    grid size.  A tensor of n elements owns ceil(n / chunk) chunks (none when it is empty)."""
    starts = [0]
    for n in numels:
        starts.append(starts[-1] + -(-int(n) // chunk))
    return starts


def chunk_of(chunk_start, c, numels, chunk=CHUNK):
    """(tensor, first element, element count) of workgroup `c`: the kernel's bisection, restated."""
    lo, hi = 0, len(numels)
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if chunk_start[mid] <= c:
            lo = mid
        else:
            hi = mid
    off = (c - chunk_start[lo]) * chunk
    return lo, off, max(0, min(chunk, numels[lo] - off))


def _refuse_param(p, device):
    if not isinstance(p, torch.Tensor):
        raise TypeError(f"optim.AdamW: parameters must be tensors, got {type(p)}")
    if p.dtype != torch.float32:
        raise TypeError(f"optim.AdamW: parameters must be float32, got {p.dtype}")
    if p.layout != torch.strided or not p.is_contiguous():
        raise ValueError("optim.AdamW: parameters must be dense and contiguous")
    if device is not None and p.device != device:
        raise ValueError(f"optim.AdamW: parameters on more than one device ({device} and {p.device})")
    if not p.is_cuda:
        raise _lib.HipLibraryError(f"optim.AdamW: a parameter lives on {p.device}: the HIP step needs device tensors (no CPU fallback)")


def _refuse_grad(g, p, device):
    """The refusal for a gradient step() cannot take (its own loop tests the same conditions inline)."""
    if g.layout != torch.strided:
        raise RuntimeError("optim.AdamW does not support sparse gradients")
    if g.dtype != torch.float32 or g.device != device or not g.is_contiguous() or g.shape != p.shape:
        raise TypeError(f"optim.AdamW: a gradient must be a contiguous float32 tensor of its parameter's shape on {device}, got "
                        f"{g.dtype} {tuple(g.shape)} (strides {g.stride()}) on {g.device}")


class AdamW(torch.optim.Optimizer):
    _step_supports_amp_scaling = True   # GradScaler.step sets self.grad_scale / self.found_inf and does not synchronise

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None):
        if isinstance(lr, torch.Tensor):
            raise ValueError("optim.AdamW: lr must be a Python number (the group table is passed to the kernel by value)")
        if amsgrad or maximize or differentiable or capturable or foreach or fused:
            raise NotImplementedError("optim.AdamW implements plain AdamW only: amsgrad, maximize, differentiable, capturable, "
                                      "foreach and fused are refused (no fallback)")
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid betas: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        self._plan = None
        # torch.optim.AdamW's group keys, so that param_groups of a checkpoint carry over in both directions
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)

    # ---- groups ---------------------------------------------------------------------------------------------------------------

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            self._check_group(group)
            device = next((p.device for g in self.param_groups for p in g["params"]), None)
            for p in group["params"]:
                if isinstance(p, torch.Tensor) and p.device != device:
                    raise ValueError(f"optim.AdamW: parameters on more than one device ({device} and {p.device})")
            for p in group["params"]:
                _refuse_param(p, device)
        except Exception:
            self.param_groups.pop()
            raise
        if len(self.param_groups) > MAX_GROUPS:
            self.param_groups.pop()
            raise _lib.HipLibraryError(f"optim.AdamW: at most {MAX_GROUPS} parameter groups")
        self._plan = None    # the tables are rebuilt at the next step; existing state is carried over

    @staticmethod
    def _check_group(group):
        if group.get("amsgrad") or group.get("maximize") or group.get("differentiable") or group.get("capturable") \
                or group.get("foreach") or group.get("fused"):
            raise NotImplementedError("optim.AdamW implements plain AdamW only: amsgrad, maximize, differentiable, capturable, "
                                      "foreach and fused are refused (no fallback)")
        if isinstance(group["lr"], torch.Tensor):
            raise ValueError("optim.AdamW: lr must be a Python number")

    # ---- tables and state -----------------------------------------------------------------------------------------------------

    def _build_plan(self):
        """Device tables for the current parameter list; state that exists (an earlier plan's, or what load_state_dict
        left in self.state) is copied into the new flat buffers.  Allocates and may synchronise: first step, and the first
        step after add_param_group / load_state_dict only."""
        params, group_of = [], []
        for gi, g in enumerate(self.param_groups):
            self._check_group(g)
            for p in g["params"]:
                params.append(p)
                group_of.append(gi)
        if not params:
            raise ValueError("optim.AdamW: no parameters")
        device = params[0].device
        for p in params:
            _refuse_param(p, device)
        T = len(params)
        numels = [p.numel() for p in params]
        starts = chunk_plan(numels)
        if starts[-1] >= 2 ** 31:
            raise _lib.HipLibraryError("optim.AdamW: more chunks than a launch grid holds")
        offs, total = [], 0
        for n in numels:
            offs.append(total)
            total += -(-n // _ALIGN) * _ALIGN
        with torch.no_grad():
            exp_avg = torch.zeros(max(total, _ALIGN), dtype=torch.float32, device=device)
            exp_avg_sq = torch.zeros_like(exp_avg)
            steps_host = torch.zeros(T, dtype=torch.float32)
            for i, p in enumerate(params):
                old = self.state.get(p)
                if old:
                    exp_avg[offs[i]:offs[i] + numels[i]].copy_(old["exp_avg"].reshape(-1))
                    exp_avg_sq[offs[i]:offs[i] + numels[i]].copy_(old["exp_avg_sq"].reshape(-1))
                    steps_host[i] = float(old["step"])
            steps = steps_host.to(device)
            for i, p in enumerate(params):
                self.state[p] = {"step": steps[i],
                                 "exp_avg": exp_avg[offs[i]:offs[i] + numels[i]].view(p.shape),
                                 "exp_avg_sq": exp_avg_sq[offs[i]:offs[i] + numels[i]].view(p.shape)}

            def table(values, dtype):
                return torch.tensor(values, dtype=dtype).to(device)
            plan = dict(
                params=params, device=device, T=T, numels=numels, num_chunks=starts[-1],
                addresses=[p.data_ptr() for p in params],
                exp_avg=exp_avg, exp_avg_sq=exp_avg_sq, steps=steps,
                p_ptrs=table([p.data_ptr() for p in params], torch.int64),
                m_ptrs=table([exp_avg.data_ptr() + 4 * o for o in offs], torch.int64),
                v_ptrs=table([exp_avg_sq.data_ptr() + 4 * o for o in offs], torch.int64),
                numel=table(numels, torch.int64),
                chunk_start=table(starts, torch.int32),
                group=table(group_of, torch.int32),
                g_ptrs=torch.zeros(T, dtype=torch.int64, device=device),
                scalars=torch.zeros(2 * T, dtype=torch.float32, device=device),
                ring=[torch.zeros(T, dtype=torch.int64).pin_memory() for _ in range(RING_SLOTS)],
                events=[None] * RING_SLOTS, slot=0,
                groups_host=(C.c_double * (5 * len(self.param_groups)))(),
            )
            plan["ring_np"] = [r.numpy() for r in plan["ring"]]
        self._plan = plan
        return plan

    def _plan_is_current(self, plan):
        n = 0
        for g in self.param_groups:
            n += len(g["params"])
        return n == plan["T"]

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        plan = self._plan
        if plan is None or not self._plan_is_current(plan):
            plan = self._build_plan()
        params, device = plan["params"], plan["device"]
        f32, strided = torch.float32, torch.strided
        ptrs, touched = [], []
        for p, address in zip(params, plan["addresses"]):
            g = p.grad
            if g is None:
                ptrs.append(0)
                continue
            if g.layout is not strided or g.dtype is not f32 or g.device != device or not g.is_contiguous() or g.shape != p.shape:
                _refuse_grad(g, p, device)
            if p.data_ptr() != address:
                # (a parameter whose storage was replaced: module.to(), p.data = ...)
                raise _lib.HipLibraryError("optim.AdamW: a parameter moved to other memory since the optimiser was built; "
                                           "build a new optimiser (load_state_dict carries the state over)")
            ptrs.append(g.data_ptr())
            touched.append(p)
        if not touched:
            return loss
        gh = plan["groups_host"]
        for gi, grp in enumerate(self.param_groups):
            self._check_group(grp)
            b1, b2 = grp["betas"]
            gh[5 * gi:5 * gi + 5] = [float(grp["lr"]), float(b1), float(b2), float(grp["eps"]), float(grp["weight_decay"])]
        # the slot's earlier copy has long finished unless the host runs RING_SLOTS steps ahead of the device: then wait
        slot = plan["slot"]
        plan["slot"] = (slot + 1) % RING_SLOTS
        ev = plan["events"][slot]
        if ev is not None and not ev.query():
            ev.synchronize()
        plan["ring_np"][slot][:] = ptrs
        with _lib.on_device(device):
            plan["g_ptrs"].copy_(plan["ring"][slot], non_blocking=True)
            if ev is None:
                ev = plan["events"][slot] = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(device))
            grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
            for name, t in (("grad_scale", grad_scale), ("found_inf", found_inf)):
                if t is not None and (t.dtype is not f32 or t.device != device or t.numel() != 1):
                    raise TypeError(f"optim.AdamW: {name} must be one float32 value on {device}")
            rc = _lib.lib().sr_adamw_step(
                plan["p_ptrs"].data_ptr(), plan["g_ptrs"].data_ptr(), plan["m_ptrs"].data_ptr(), plan["v_ptrs"].data_ptr(),
                plan["numel"].data_ptr(), plan["chunk_start"].data_ptr(), plan["group"].data_ptr(), plan["steps"].data_ptr(),
                plan["scalars"].data_ptr(), plan["T"], plan["num_chunks"], C.addressof(gh), len(self.param_groups),
                _lib.ptr(grad_scale), _lib.ptr(found_inf), _lib.stream_ptr(device))
        _lib.check(rc, "sr_adamw_step")
        # the kernel wrote through raw pointers: what is keyed on _version (packed weights, captured graphs) must see it
        torch.autograd.graph.increment_version(touched)
        return loss

    # ---- checkpoints ----------------------------------------------------------------------------------------------------------

    def state_dict(self):
        """torch.optim.AdamW's schema.  Entries are copies (the live state is views of flat buffers), `step` a 0-dim fp32
        host tensor as torch keeps it; parameters that never had a gradient have no entry, as in torch.  Synchronises."""
        sd = super().state_dict()
        state = {}
        for k, s in sd["state"].items():
            step = s["step"].detach().to("cpu", torch.float32).clone()
            if float(step) == 0.0:
                continue
            state[k] = {"step": step, "exp_avg": s["exp_avg"].detach().clone(), "exp_avg_sq": s["exp_avg_sq"].detach().clone()}
        sd["state"] = state
        return sd

    def load_state_dict(self, state_dict):
        """Takes a state_dict of this class or of torch.optim.AdamW (amsgrad / maximize checkpoints are refused)."""
        for g in state_dict["param_groups"]:
            self._check_group({"lr": 0.0, **g})
        if any("max_exp_avg_sq" in s for s in state_dict["state"].values()):
            raise NotImplementedError("optim.AdamW: the checkpoint holds amsgrad state")
        super().load_state_dict(state_dict)    # (self.state now holds the checkpoint's entries and nothing else)
        for g in self.param_groups:
            g.setdefault("decoupled_weight_decay", True)
        self._plan = None
        self._build_plan()                     # parameters without an entry start from zero
