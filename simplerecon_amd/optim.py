"""The optimiser step of the training path: multi-tensor AdamW on the HIP kernels of csrc/sr_optim.hip
(include/simplerecon_hip.h, section "optimiser").

    opt = optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    loss.backward(); opt.step()                     # two launches for every parameter tensor of the model
    scaler.step(opt); scaler.update()               # torch.amp.GradScaler: unscale and skip inside the kernel, no host sync

    opt = optim.AdamW(model.parameters(), max_grad_norm=1.0)      # global-norm clipping inside the step: four launches
    scaler = optim.LossScaler(init_scale=2.0 ** 10)               # inf check and scale update in the same four
    scaler.scale(loss).backward(); scaler.step(opt); scaler.update()
    opt.grad_norm, opt.grad_norms, opt.clip_coef, opt.found_inf_last         # fp32 device tensors, overwritten each step

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

Gradient statistics (`max_grad_norm=`, `grad_stats=True`, or a step through optim.LossScaler): sr_grad_stats reads every
gradient once, behind the address upload, and leaves per-tensor L2 norms, the global norm, the non-finite flag and torch's
clip coefficient on the device; the AdamW pass multiplies the coefficient in registers as it divides by the scale.  All
parameters of the optimiser are clipped together, whatever their group.  Norms refer to the unscaled gradient: under a
torch.amp.GradScaler the pass takes `grad_scale` from the scaler.  Without a scaler a non-finite gradient is not a reason
to skip: the coefficient is NaN and so are the parameters afterwards, as after torch's clip_grad_norm_.

optim.LossScaler is torch.amp.GradScaler for optim.AdamW: same constructor defaults, same state_dict, same update rule
(torch's _amp_update_scale_), but the inf check is the statistics pass and the scale update runs at the end of its
second launch, so nothing ever writes a gradient.  It serves one optimiser per iteration.

optim.clip_grad_norm_ is torch.nn.utils.clip_grad_norm_ for contiguous fp32 device gradients (statistics, then one in-place
multiply); optim.grad_stats_reference restates the statistics in float64 on the host.

Out of scope: other norms than L2, per-group and value clipping, error_if_nonfinite, writing packed or 16-bit weights from
inside the kernel, HIP-graph capture of the step, 16-bit parameters and sharded state."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib

CHUNK = 4096        # SR_ADAMW_CHUNK: elements one workgroup updates
MAX_GROUPS = 16     # SR_ADAMW_MAX_GROUPS
RING_SLOTS = 8      # pinned gradient-address tables in flight
_ALIGN = 4          # state views start at multiples of 4 elements: 16-byte accesses whenever p and g allow them
_NORM, _FOUND_INF, _COEF, _SCALE, _SLOTS = 0, 1, 2, 3, 4   # SR_GRAD_STATS_*: the slots of the statistics pass's `stats`


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


class _GradTables:
    """What the multi-tensor launches over a list of gradients need on the device: sizes, the chunk prefix table, the
    gradient-address table with its ring of pinned host copies, and the workspace and outputs of the statistics pass.
    Building it allocates and may synchronise; upload(), stats() and scale_inplace() do neither."""

    def __init__(self, numels, device):
        starts = chunk_plan(numels)
        if starts[-1] >= 2 ** 31:
            raise _lib.HipLibraryError("optim.AdamW: more chunks than a launch grid holds")
        T = len(numels)
        self.T, self.numels, self.num_chunks, self.device = T, list(numels), starts[-1], device
        self.numel = torch.tensor(self.numels, dtype=torch.int64).to(device)
        self.chunk_start = torch.tensor(starts, dtype=torch.int32).to(device)
        self.g_ptrs = torch.zeros(T, dtype=torch.int64, device=device)
        self.ring = [torch.zeros(T, dtype=torch.int64).pin_memory() for _ in range(RING_SLOTS)]
        self.ring_np = [r.numpy() for r in self.ring]
        self.events, self.slot = [None] * RING_SLOTS, 0
        self.workspace_bytes = _lib.lib().sr_grad_stats_workspace_bytes(self.num_chunks, T)
        self.workspace = torch.empty(self.workspace_bytes // 8, dtype=torch.float64, device=device)
        self.norms = torch.empty(T, dtype=torch.float32, device=device)
        self.stats_out = torch.empty(_SLOTS, dtype=torch.float32, device=device)
        self.stats_ran = False

    def upload(self, ptrs):
        """Gradient addresses (0 = no gradient) to the device in one asynchronous copy on the current stream, `device`
        being current.  The slot's earlier copy has long finished unless the host runs RING_SLOTS steps ahead of the
        device: then wait."""
        slot = self.slot
        self.slot = (slot + 1) % RING_SLOTS
        ev = self.events[slot]
        if ev is not None and not ev.query():
            ev.synchronize()
        self.ring_np[slot][:] = ptrs
        self.g_ptrs.copy_(self.ring[slot], non_blocking=True)
        if ev is None:
            ev = self.events[slot] = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))

    def stats(self, grad_scale=None, max_norm=None, scaler=None):
        """The statistics pass over the uploaded addresses: norms, stats_out and, with a LossScaler, its update."""
        scale, tracker = (scaler._scale, scaler._growth_tracker) if scaler is not None else (None, None)
        rc = _lib.lib().sr_grad_stats(
            self.g_ptrs.data_ptr(), self.numel.data_ptr(), self.chunk_start.data_ptr(), self.T, self.num_chunks,
            _lib.ptr(grad_scale), float(max_norm or 0.0), self.norms.data_ptr(), self.stats_out.data_ptr(), _lib.ptr(scale),
            _lib.ptr(tracker), scaler._growth_factor if scaler is not None else 1.0,
            scaler._backoff_factor if scaler is not None else 1.0, scaler._growth_interval if scaler is not None else 1,
            self.workspace.data_ptr(), self.workspace_bytes, _lib.stream_ptr(self.device))
        _lib.check(rc, "sr_grad_stats")
        self.stats_ran = True

    def scale_inplace(self, coef):
        rc = _lib.lib().sr_grad_scale_inplace(self.g_ptrs.data_ptr(), self.numel.data_ptr(), self.chunk_start.data_ptr(),
                                              self.T, self.num_chunks, coef.data_ptr(), _lib.stream_ptr(self.device))
        _lib.check(rc, "sr_grad_scale_inplace")


def _check_max_norm(max_norm):
    max_norm = float(max_norm)
    if not max_norm > 0.0 or math.isinf(max_norm) or not float(np.float32(max_norm)) > 0.0:    # (the kernel takes it as fp32)
        raise ValueError(f"optim: max_norm must be a positive finite number, got {max_norm}")
    return max_norm


class AdamW(torch.optim.Optimizer):
    _step_supports_amp_scaling = True   # GradScaler.step sets self.grad_scale / self.found_inf and does not synchronise

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, *, maximize=False,
                 foreach=None, capturable=False, differentiable=False, fused=None, max_grad_norm=None, grad_stats=False):
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
        self.max_grad_norm = None if max_grad_norm is None else _check_max_norm(max_grad_norm)
        self.grad_stats = bool(grad_stats)
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
        tables = _GradTables(numels, device)
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
                params=params, device=device, T=T, numels=numels, num_chunks=tables.num_chunks, tables=tables,
                addresses=[p.data_ptr() for p in params],
                exp_avg=exp_avg, exp_avg_sq=exp_avg_sq, steps=steps,
                p_ptrs=table([p.data_ptr() for p in params], torch.int64),
                m_ptrs=table([exp_avg.data_ptr() + 4 * o for o in offs], torch.int64),
                v_ptrs=table([exp_avg_sq.data_ptr() + 4 * o for o in offs], torch.int64),
                numel=tables.numel, chunk_start=tables.chunk_start, g_ptrs=tables.g_ptrs,
                group=table(group_of, torch.int32),
                scalars=torch.zeros(2 * T, dtype=torch.float32, device=device),
                groups_host=(C.c_double * (5 * len(self.param_groups)))(),
            )
        self._plan = plan
        return plan

    def _plan_is_current(self, plan):
        n = 0
        for g in self.param_groups:
            n += len(g["params"])
        return n == plan["T"]

    # ---- gradient statistics of the last step that ran the pass (None before the first) -------------------------------------------

    def _stat(self, slot):
        tables = self._plan["tables"] if self._plan is not None else None
        return tables.stats_out[slot] if tables is not None and tables.stats_ran else None

    @property
    def grad_norm(self):
        """Global L2 norm of the unscaled gradients: a 0-dim fp32 device tensor, overwritten by the next step."""
        return self._stat(_NORM)

    @property
    def grad_norms(self):
        """Per-tensor L2 norms, [T] in parameter order (groups in order), 0 where a parameter had no gradient."""
        tables = self._plan["tables"] if self._plan is not None else None
        return tables.norms if tables is not None and tables.stats_ran else None

    @property
    def clip_coef(self):
        """What the step multiplied every gradient by: min(1, max_grad_norm / (grad_norm + 1e-6)); 1 without clipping."""
        return self._stat(_COEF)

    @property
    def found_inf_last(self):
        """1.0 when some gradient element of the last step was not finite, else 0.0."""
        return self._stat(_FOUND_INF)

    @torch.no_grad()
    def step(self, closure=None, *, loss_scaler=None):
        """loss_scaler: the optim.LossScaler whose step() this is (its callers use scaler.step(optimizer))."""
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
        tables = plan["tables"]
        grad_scale, found_inf = getattr(self, "grad_scale", None), getattr(self, "found_inf", None)
        for name, t in (("grad_scale", grad_scale), ("found_inf", found_inf)):
            if t is not None and (t.dtype is not f32 or t.device != device or t.numel() != 1):
                raise TypeError(f"optim.AdamW: {name} must be one float32 value on {device}")
        if loss_scaler is not None:
            if grad_scale is not None or found_inf is not None:
                raise RuntimeError("optim.AdamW: a step through optim.LossScaler inside a torch.amp.GradScaler step")
            loss_scaler._device_state(device)
        with _lib.on_device(device):
            tables.upload(ptrs)
            coef = None
            if loss_scaler is not None or self.max_grad_norm is not None or self.grad_stats:
                tables.stats(grad_scale, self.max_grad_norm, loss_scaler)
                out = tables.stats_out
                if loss_scaler is not None:
                    # (the scaler's own slot already holds the next step's scale: divide by the scale of this one)
                    grad_scale, found_inf = out[_SCALE], out[_FOUND_INF]
                if self.max_grad_norm is not None:
                    coef = out[_COEF]
            if coef is None:
                rc = _lib.lib().sr_adamw_step(
                    plan["p_ptrs"].data_ptr(), plan["g_ptrs"].data_ptr(), plan["m_ptrs"].data_ptr(), plan["v_ptrs"].data_ptr(),
                    plan["numel"].data_ptr(), plan["chunk_start"].data_ptr(), plan["group"].data_ptr(), plan["steps"].data_ptr(),
                    plan["scalars"].data_ptr(), plan["T"], plan["num_chunks"], C.addressof(gh), len(self.param_groups),
                    _lib.ptr(grad_scale), _lib.ptr(found_inf), _lib.stream_ptr(device))
            else:
                rc = _lib.lib().sr_adamw_step_clipped(
                    plan["p_ptrs"].data_ptr(), plan["g_ptrs"].data_ptr(), plan["m_ptrs"].data_ptr(), plan["v_ptrs"].data_ptr(),
                    plan["numel"].data_ptr(), plan["chunk_start"].data_ptr(), plan["group"].data_ptr(), plan["steps"].data_ptr(),
                    plan["scalars"].data_ptr(), plan["T"], plan["num_chunks"], C.addressof(gh), len(self.param_groups),
                    _lib.ptr(grad_scale), _lib.ptr(found_inf), _lib.ptr(coef), _lib.stream_ptr(device))
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


# ---- loss scaler ------------------------------------------------------------------------------------------------------------------

class LossScaler:
    """torch.amp.GradScaler for optim.AdamW with the inf check, the unscale and the scale update on the HIP kernels.

        scaler = optim.LossScaler(init_scale=2.0 ** 10)
        scaler.scale(loss).backward(); scaler.step(opt); scaler.update()

    Scale (fp32) and growth tracker (int32) live on the device, created at the first scale() or step().  step() makes the
    optimiser run the statistics pass, whose second launch raises the flag, keeps the scale of this step for the AdamW
    pass and applies torch's _amp_update_scale_ to the scaler's own slots; update() therefore only closes the iteration.
    One optimiser per iteration: a second step() before update() raises, as torch does for the same optimiser."""

    def __init__(self, device="cuda", init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
        if not growth_factor > 1.0:
            raise ValueError("The growth factor must be > 1.0.")
        if not 0.0 < backoff_factor < 1.0:
            raise ValueError("The backoff factor must be in (0, 1).")
        if int(growth_interval) < 1:
            raise ValueError("optim.LossScaler: growth_interval must be at least 1")
        if torch.device(device).type != "cuda":
            raise _lib.HipLibraryError(f"optim.LossScaler: device {device}: the scaler's state lives on a HIP device")
        self._init_scale, self._init_growth_tracker = float(init_scale), 0
        self._growth_factor, self._backoff_factor = float(growth_factor), float(backoff_factor)
        self._growth_interval = int(growth_interval)
        self._scale = self._growth_tracker = None
        self._stepped = False

    def _device_state(self, device):
        if self._scale is None:
            self._scale = torch.full((), self._init_scale, dtype=torch.float32, device=device)
            self._growth_tracker = torch.full((), self._init_growth_tracker, dtype=torch.int32, device=device)
        elif self._scale.device != device:
            raise ValueError(f"optim.LossScaler: its state lives on {self._scale.device}, not on {device}")

    def scale(self, loss):
        """loss * scale, on the device (no synchronisation)."""
        if not isinstance(loss, torch.Tensor) or not loss.is_cuda:
            raise _lib.HipLibraryError("optim.LossScaler.scale takes a device tensor (no CPU fallback)")
        self._device_state(loss.device)
        return loss * self._scale

    def step(self, optimizer, *args, **kwargs):
        if not isinstance(optimizer, AdamW):
            raise TypeError(f"optim.LossScaler steps optim.AdamW only, got {type(optimizer).__name__} (no fallback)")
        if "closure" in kwargs or args:
            raise RuntimeError("Closure use is not currently supported if GradScaler is enabled.")
        if self._stepped:
            raise RuntimeError("step() has already been called since the last update().")
        self._stepped = True
        return optimizer.step(loss_scaler=self)

    def update(self, new_scale=None):
        """Closes the iteration (the device applied the update rule inside step()).  A second update() without a step()
        in between changes nothing.  new_scale: a number that replaces the scale."""
        if new_scale is not None:
            if self._scale is None:
                self._init_scale = float(new_scale)
            else:
                self._scale.fill_(float(new_scale))
        self._stepped = False

    def get_scale(self):
        """The current scale as a Python float.  Synchronises, as torch's does."""
        return self._init_scale if self._scale is None else float(self._scale)

    def _get_growth_tracker(self):
        return self._init_growth_tracker if self._growth_tracker is None else int(self._growth_tracker)

    def get_growth_factor(self):
        return self._growth_factor

    def get_backoff_factor(self):
        return self._backoff_factor

    def get_growth_interval(self):
        return self._growth_interval

    def state_dict(self):
        """torch.amp.GradScaler's schema: a checkpoint moves between the two classes in both directions."""
        return {"scale": self.get_scale(), "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": self._get_growth_tracker()}

    def load_state_dict(self, state_dict):
        if len(state_dict) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved from a disabled instance "
                               "of GradScaler.")
        self._init_scale = float(state_dict["scale"])
        self._growth_factor = float(state_dict["growth_factor"])
        self._backoff_factor = float(state_dict["backoff_factor"])
        self._growth_interval = int(state_dict["growth_interval"])
        self._init_growth_tracker = int(state_dict["_growth_tracker"])
        if self._scale is not None:
            self._scale.fill_(self._init_scale)
            self._growth_tracker.fill_(self._init_growth_tracker)


# ---- torch.nn.utils.clip_grad_norm_ ---------------------------------------------------------------------------------------------

_CLIP_TABLES = {}        # (device, sizes) -> _GradTables of clip_grad_norm_: a repeated call allocates no table
_CLIP_TABLES_KEPT = 4


def clip_grad_norm_(parameters, max_norm, norm_type=2.0):
    """torch.nn.utils.clip_grad_norm_ for contiguous fp32 device gradients: the statistics pass, then one in-place multiply
    by min(1, max_norm / (norm + 1e-6)) (always, as torch multiplies).  Returns the total norm as a 0-dim device tensor
    and does not synchronise; a repeated call on the same parameter sizes builds no table."""
    if float(norm_type) != 2.0:
        raise NotImplementedError(f"optim.clip_grad_norm_ implements the L2 norm only, got norm_type={norm_type} (no fallback)")
    max_norm = _check_max_norm(max_norm)
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    params = [p for p in parameters if p.grad is not None]
    if not params:
        return torch.zeros(())
    device = params[0].grad.device
    for p in params:
        g = p.grad
        if g.layout is not torch.strided or g.dtype is not torch.float32 or g.device != device or not g.is_contiguous() \
                or g.shape != p.shape:
            _refuse_grad(g, p, device)
    if device.type != "cuda":
        raise _lib.HipLibraryError(f"optim.clip_grad_norm_: gradients live on {device}: the HIP pass needs device tensors "
                                   "(no CPU fallback)")
    key = (device, tuple(p.numel() for p in params))
    tables = _CLIP_TABLES.pop(key, None)
    if tables is None:
        tables = _GradTables(key[1], device)
        while len(_CLIP_TABLES) >= _CLIP_TABLES_KEPT:
            del _CLIP_TABLES[next(iter(_CLIP_TABLES))]
    _CLIP_TABLES[key] = tables       # (most recently used last)
    with torch.no_grad(), _lib.on_device(device):
        tables.upload([p.grad.data_ptr() for p in params])
        tables.stats(None, max_norm)
        tables.scale_inplace(tables.stats_out[_COEF])
        return tables.stats_out[_NORM].clone()


def grad_stats_reference(grads, scale=1.0, max_norm=None):
    """The statistics pass restated in float64 on the host: (per-tensor norms [T], total norm, found_inf, clip coefficient)
    of the gradients divided by `scale`; None in `grads` is a tensor without a gradient (norm 0).  The coefficient is
    min(1, max_norm / (total + 1e-6)) in float64, 1.0 without a max_norm."""
    sums = []
    for g in grads:
        if g is None:
            sums.append(0.0)
            continue
        x = g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else np.asarray(g)
        x = x.astype(np.float64).reshape(-1)
        with np.errstate(over="ignore", invalid="ignore"):
            sums.append(float(np.sum(x * x)))
    sums = np.asarray(sums, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        total_sum = float(np.sum(sums))
        norms = np.sqrt(sums) / float(scale)
        total = float(np.sqrt(total_sum) / float(scale))
        coef = 1.0
        if max_norm is not None:
            coef = float(max_norm) / (total + 1e-6)
            coef = 1.0 if coef > 1.0 else coef
    return norms, total, 0.0 if math.isfinite(total_sum) else 1.0, coef
