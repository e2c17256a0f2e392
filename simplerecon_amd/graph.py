"""HIP-graph replay of a launch-bound step.

One keyframe batch is ~230 kernel launches (matching encoder + plane sweep + 165 convs); at batch 1 the Python /
ctypes submission of those launches (~6 ms) is as long as the GPU work.  `GraphedCallable` records the launches of
`fn(*inputs)` once into a HIP graph (`torch.cuda.CUDAGraph` is hipGraph on ROCm) and replays it: one submission per
step, no per-launch host work, back-to-back kernels on the device.

Everything the HIP path launches goes to torch's current stream (`_lib.stream_ptr`), so capture needs no special
casing; the library itself never allocates or synchronises.  Packed-weight caches and workspaces are filled by the
warm-up runs before the capture, inside it they are only read.

The graph bakes in the ADDRESSES of those packed weights, which live outside its memory pool: the GraphedCallable keeps a
reference to every payload cached at capture time, so that an eager call which re-packs after a weight update (and drops the
cache's own reference) cannot leave a replay reading recycled memory.  A replay still computes with the weights as they were
packed at capture -- mixed with whatever the graph reads live (biases, the sweep's MLP weights) -- so with `check_weights`
a replay after any change of a parameter or buffer raises instead.
"""
import torch

from . import ops


class StaleGraphError(RuntimeError):
    """A captured graph was replayed after the weights it was captured with changed."""


def _weight_state(modules):
    """[(the module's own dict, name, qualified name, version, address)] of every parameter and buffer of `modules` (roots),
    each once.  The qualified name (`ClassOfTheRoot.path.to.module.weight`) is for the error message only."""
    state, seen = [], set()
    for root in modules:
        for path, m in root.named_modules():
            for d in (m._parameters, m._buffers):
                for name, t in d.items():
                    if t is None or id(t) in seen:
                        continue
                    seen.add(id(t))
                    try:
                        version = t._version
                    except RuntimeError:   # a tensor made in inference mode carries no version counter: address only
                        version = None
                    state.append((d, name, ".".join(filter(None, (type(root).__name__, path, name))), version, t.data_ptr()))
    return state


def _flatten(x, out):
    if isinstance(x, torch.Tensor):
        out.append(x)
    elif isinstance(x, (list, tuple)):
        for v in x:
            _flatten(v, out)
    elif isinstance(x, dict):
        for k in x:
            _flatten(x[k], out)
    elif x is not None and not isinstance(x, (bool, int, float, str)):
        raise TypeError(f"GraphedCallable inputs must be tensors / lists / dicts / scalars, got {type(x)}")
    return out


def _clone_like(x):
    if isinstance(x, torch.Tensor):
        return x.clone(memory_format=torch.preserve_format)
    if isinstance(x, (list, tuple)):
        return type(x)(_clone_like(v) for v in x)
    if isinstance(x, dict):
        return {k: _clone_like(v) for k, v in x.items()}
    return x


class GraphedCallable:
    """`g = GraphedCallable(fn, *example_inputs)`; `out = g(*inputs)` copies `inputs` into the captured input
    buffers (device-to-device, skipped for tensors that already ARE those buffers: see `static_inputs`) and replays the
    graph.  The returned tensors are the graph's static output buffers: they are overwritten by the next call.
    Shapes, dtypes, devices and non-tensor arguments are frozen at capture time.

    `modules`: the nn.Modules `fn` runs (roots).  The payloads the packed-weight cache holds for them after the capture are
    kept alive with the graph.  With modules=None that is every payload of the process-wide cache, whichever module it
    belongs to: harmless for the result, but the packed weights of unrelated models then stay allocated for as long as this
    graph lives -- name the modules where that matters (DepthModel.graphed does).  check_weights=True (needs `modules`): (version, address) of
    every parameter and buffer is recorded at capture and compared before each replay; a difference raises StaleGraphError
    -- capture again.  check_weights=False replays whatever was packed at capture."""

    def __init__(self, fn, *example_inputs, warmup=3, modules=None, check_weights=False):
        if check_weights and modules is None:
            raise ValueError("check_weights needs the `modules` whose weights the graph reads")
        modules = None if modules is None else list(modules)
        flat = _flatten(example_inputs, [])
        if not flat or not all(t.is_cuda for t in flat):
            raise ValueError("GraphedCallable needs device tensors as inputs")
        self.device = flat[0].device
        self.static_inputs = _clone_like(example_inputs)
        self._static_flat = _flatten(self.static_inputs, [])
        self._shapes = [(tuple(t.shape), t.dtype) for t in self._static_flat]
        with torch.cuda.device(self.device), torch.inference_mode():
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(side):
                for _ in range(max(1, warmup)):   # fills weight-pack caches and workspaces outside the capture
                    fn(*self.static_inputs)
            torch.cuda.current_stream(self.device).wait_stream(side)
            torch.cuda.synchronize(self.device)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                self.static_outputs = fn(*self.static_inputs)
        self._pinned = ops.packed_payloads(modules)
        self._forget_epoch = ops._FORGET_EPOCH
        self._weights = _weight_state(modules) if check_weights else None

    def _check_weights(self):
        for d, name, qualified, version, address in self._weights:
            t = d.get(name)
            if t is None or t.data_ptr() != address or (version is not None and t._version != version):
                raise StaleGraphError(f"parameter or buffer `{qualified}` changed since this graph was captured: a replay would "
                                      "compute with the weights packed at capture.  Capture again (DepthModel.graphed / "
                                      "GraphedCallable), or pass check_weights=False to replay the captured weights")

    def __call__(self, *inputs):
        flat = _flatten(inputs, [])
        if len(flat) != len(self._static_flat):
            raise ValueError(f"expected {len(self._static_flat)} input tensors, got {len(flat)}")
        if self._forget_epoch != ops._FORGET_EPOCH:
            raise StaleGraphError("ops.forget_packed() was called since this graph was captured: it still reads the payloads "
                                  "packed before.  Capture again")
        if self._weights is not None:
            self._check_weights()
        with torch.inference_mode():
            for dst, src, (shape, dtype) in zip(self._static_flat, flat, self._shapes):
                if src is dst:
                    continue
                if tuple(src.shape) != shape or src.dtype != dtype:
                    raise ValueError(f"input of shape {tuple(src.shape)} / {src.dtype} does not match the captured "
                                     f"{shape} / {dtype}")
                dst.copy_(src, non_blocking=True)
            self.graph.replay()
        return self.static_outputs
