"""The inference schedule of DepthModel.forward_tensors as a trace: which launches go out, in which order, on which HIP
stream, behind which waits.  Shared by tests/test_gpu_schedule_trace.py and scripts/record_decoder_schedule_trace.py.
The fork / join logic only runs on a GPU, so the traces are taken (and the fixture was recorded) on the MI355X.

A trace is a list of records in program order, from the entry of forward_tensors to its return:
  [op, module, stream, [C, H, W, channel offset inside its pixel, pixel stride]]   ops.conv2d / upsample2x / copy_into / exp:
      the qualified name of the module whose weights the call uses (or None), the label of the current stream and where the
      result lies -- a slice of a concat buffer differs from a fresh tensor in the last two numbers.  No addresses, no entry
      points: those depend on the allocator and on the launch plan.  Launches made while the image-prior side stream is current
      are the image-prior encoder's own and are left out.
  ["cost_volume", "cost_volume", stream, [...], reserve_cus]                       the cost-volume manager's call
  ["wait_stream", waiter, waited] / ["wait_event", waiter, event ordinal] / ["record", event ordinal]
      ordinals count the events recorded on the image-prior stream; an event recorded elsewhere has none (None).
followed by one ["outputs", [[key, None | [shape, dtype, requires_grad]], ...]].
Streams are labelled by identity: main (current at entry), dec1 / dec2 (DepthDecoderPP._side_streams), prior
(DepthModel._prior_streams), sub0.. (DepthModel._streams)."""
import contextlib
import gzip
import json
import os

import pytest
import torch

from simplerecon_amd import depth_model as dm
from simplerecon_amd import networks, ops, synthetic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decoder_schedule_trace.json.gz")
DEV = torch.device("cuda", 0)
K, D, H4, W4 = 2, 8, 24, 32   # 96 x 128 images: decoder nodes see 48x64, 24x32, 12x16 and 6x8 maps

# case -> (batch, attributes set on the model, ...).  At B = 3 the fork rule's `regions` are 72 / 18 / 6 / 3, so a limit of 10
# makes levels 2 and 3 fork and levels 0 and 1 not.
CASES = {
    "A": dict(B=1, side=True),
    "B": dict(B=1, side=False),
    "C": dict(B=3, side=True, max_regions=10),
    "D": dict(B=3, side=False, max_regions=10),
    "E": dict(B=3, side=True, max_regions=0),
    "F": dict(B=3, side=False, max_regions=0),
    "G": dict(B=1, side=True, no_level_events=True),
    "H": dict(B=4, side=True, num_streams=2),
    "I": dict(B=1, side=True, fvt="simple_cost_volume"),
    "L": dict(B=1, side=True, train=True),
}
EQUAL_OUTPUTS = (("A", "B", "G"), ("C", "D", "E", "F"))


def build_model(fvt="mlp_feature_volume"):
    opts = dm.default_options(image_width=4 * W4, image_height=4 * H4, model_num_views=K + 1, matching_num_depth_bins=D,
                              feature_volume_type=fvt)
    model = dm.DepthModel(opts)
    synthetic.seeded_fill_(model.encoder, seed=9, gain=1.0)
    for i, m in enumerate((model.matching_model, model.cost_volume_net, model.depth_decoder,
                           getattr(model.cost_volume, "mlp", None))):
        if m is not None:
            synthetic.seeded_fill_(m, seed=10 + i)
    return model.to(DEV).eval()


def inputs(B):
    inp = {k: v.to(DEV) for k, v in synthetic.cost_volume_inputs(B, K, 16, H4, W4, seed=20 + B).items()}
    g = torch.Generator(device="cpu").manual_seed(20 + B)
    cur = torch.randn((B, 3, 4 * H4, 4 * W4), generator=g).to(DEV)
    src = torch.randn((B, K, 3, 4 * H4, 4 * W4), generator=g).to(DEV)
    return cur, src, inp["src_extrinsics"], inp["src_poses"], inp["src_Ks"], inp["cur_invK"]


def _where(t):
    pix = t.stride(3)
    return [t.shape[1], t.shape[2], t.shape[3], t.storage_offset() % pix if pix else 0, pix]


@contextlib.contextmanager
def tracing(model, trace):
    """Appends the records of everything `model` does inside the block to `trace`."""
    names = {id(m): n for n, m in model.named_modules()}
    main = torch.cuda.current_stream(DEV)
    events = []   # events recorded on the prior stream, kept alive so that their ids stay theirs

    def label(stream):
        known = [("main", main), ("prior", model._prior_streams.get(DEV))]
        known += zip(("dec1", "dec2"), networks._SIDE_STREAMS.get(DEV, ()))
        known += [(f"sub{i}", s) for i, s in enumerate(model._streams.get(DEV, ()))]
        return next((n for n, s in known if s is not None and s == stream), "other")

    def ordinal(event):
        return next((i for i, e in enumerate(events) if e is event), None)

    def launch(name, module_of):
        fn = getattr(ops, name)

        def wrapper(*args, **kw):
            out = fn(*args, **kw)
            stream = label(torch.cuda.current_stream(DEV))
            if stream != "prior":
                trace.append([name, names.get(id(module_of(args, kw))), stream, _where(out)])
            return out
        return wrapper

    def sweep_hook(_module, _args, kw, out):
        trace.append(["cost_volume", names[id(model.cost_volume)], label(torch.cuda.current_stream(DEV)), _where(out[0]),
                      kw.get("reserve_cus", 0)])

    wait_stream, wait_event, record = torch.cuda.Stream.wait_stream, torch.cuda.Stream.wait_event, torch.cuda.Event.record

    inside_wait_stream = []   # torch implements wait_stream as record_event + wait_event: those two are not the project's

    def traced_wait_stream(self, other):
        trace.append(["wait_stream", label(self), label(other)])
        inside_wait_stream.append(True)
        try:
            return wait_stream(self, other)
        finally:
            inside_wait_stream.pop()

    def traced_wait_event(self, event):
        if not inside_wait_stream:
            trace.append(["wait_event", label(self), ordinal(event)])
        return wait_event(self, event)

    def traced_record(self, stream=None):
        if not inside_wait_stream and label(torch.cuda.current_stream(DEV) if stream is None else stream) == "prior":
            events.append(self)
            trace.append(["record", len(events) - 1])
        return record(self, stream)

    hook = model.cost_volume.register_forward_hook(sweep_hook, with_kwargs=True)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "conv2d", launch("conv2d", lambda a, kw: kw["conv"] if "conv" in kw else a[1]))
        for name in ("upsample2x", "copy_into", "exp"):
            mp.setattr(ops, name, launch(name, lambda a, kw: None))
        mp.setattr(torch.cuda.Stream, "wait_stream", traced_wait_stream)
        mp.setattr(torch.cuda.Stream, "wait_event", traced_wait_event)
        mp.setattr(torch.cuda.Event, "record", traced_record)
        try:
            yield trace
        finally:
            hook.remove()


def run_case(model, case):
    """(trace, outputs) of one case on `model`; every attribute a case may touch is set, so cases can share a model."""
    c = CASES[case]
    model.prior_on_side_stream = c["side"]
    model.num_streams = c.get("num_streams", 1)
    model.depth_decoder.__dict__.pop("branch_stream_max_regions", None)
    if "max_regions" in c:
        model.depth_decoder.branch_stream_max_regions = c["max_regions"]
    train = c.get("train", False)
    for name, p in model.named_parameters():
        p.requires_grad_(train and name.startswith(("cost_volume_net.", "depth_decoder.")))
    args = inputs(c["B"])
    with pytest.MonkeyPatch.context() as mp, (contextlib.nullcontext() if train else torch.inference_mode()):
        if c.get("no_level_events"):
            encode = model.encoder.forward
            mp.setattr(model.encoder, "forward", lambda image, on_level=None: encode(image))
        # warm-up: weights are packed (and their fences have passed) before the traced call
        model.forward_tensors(*args, return_mask=True)
        torch.cuda.synchronize()
        with tracing(model, []) as trace:
            out = model.forward_tensors(*args, return_mask=True)
        trace.append(["outputs", [[k, None if v is None else [list(v.shape), str(v.dtype), v.requires_grad]]
                                  for k, v in out.items()]])
        torch.cuda.synchronize()
        return trace, {k: v.detach().clone() for k, v in out.items() if v is not None}


def run_cases():
    """{case: trace}, {case: outputs} of all CASES."""
    traces, outputs = {}, {}
    models = {}
    for case, c in CASES.items():
        fvt = c.get("fvt", "mlp_feature_volume")
        if fvt not in models:
            models[fvt] = build_model(fvt)
        traces[case], outputs[case] = run_case(models[fvt], case)
    return traces, outputs


def load_golden():
    with gzip.open(GOLDEN, "rb") as f:
        return json.loads(f.read().decode())


def write_golden(traces):
    with open(GOLDEN, "wb") as f, gzip.GzipFile(fileobj=f, mode="wb", mtime=0) as z:
        z.write(json.dumps(traces, sort_keys=True, separators=(",", ":")).encode())
    return os.path.getsize(GOLDEN)
