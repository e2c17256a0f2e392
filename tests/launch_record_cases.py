"""The launches whose ops.PROFILE records tests/golden/launch_records.json pins: one tiny call per kernel family, plan and
instantiation a record can name.  Shared by tests/test_gpu_launch_records.py (compares), scripts/record_launch_records.py
(records, from the commit before a change) and scripts/launch_records_vs_trace.py (checks the names against a profiler's trace).
Plans the cost model would not pick at these sizes are forced with the library's options."""
import contextlib

import torch
from torch import nn

from simplerecon_amd import _lib, autograd_ops, ops, synthetic

DEV = "cuda:0"


@contextlib.contextmanager
def _setup(options=(), **attrs):
    """Library options and ops module switches for one case; plan answers cached under other settings are dropped."""
    saved = {k: getattr(ops, k) for k in attrs}
    with contextlib.ExitStack() as stack:
        for name, value in options:
            stack.enter_context(_lib.option(name, value))
        for k, v in attrs.items():
            setattr(ops, k, v)
        ops._SHAPE_QUERIES.clear()
        try:
            yield
        finally:
            for k, v in saved.items():
                setattr(ops, k, v)
            ops._SHAPE_QUERIES.clear()


def _map(b, c, h, w, offset=0):
    """A channels-last [b, c, h, w] view; offset = 1: one element into its buffer, so no pixel row is 16-byte aligned."""
    flat = torch.zeros(b * h * w * c + offset, device=DEV)
    return flat[offset:].view(b, h, w, c).permute(0, 3, 1, 2)


def _conv(ci, co, k=3, s=1, mode="zeros"):
    return synthetic.seeded_fill_(nn.Conv2d(ci, co, k, stride=s, padding=k // 2, padding_mode=mode), seed=ci + co).to(DEV)


def _conv2d(shape, k=3, s=1, mode="zeros", in_offset=0, out_offset=0, res=False, gate=False, tf_same=False):
    b, ci, h, w, co = shape
    pads = ops.tf_same_pads(h, w, k, s) if tf_same else (k // 2,) * 4
    ho, wo = (h + pads[0] + pads[2] - k) // s + 1, (w + pads[1] + pads[3] - k) // s + 1
    ops.conv2d(_map(b, ci, h, w, in_offset), _conv(ci, co, k, s, mode), leaky=0.1, tf_same=tf_same,
               out=_map(b, co, ho, wo, out_offset) if out_offset else None, residual=_map(b, co, ho, wo) if res else None,
               gate=torch.ones(b, ci, device=DEV) if gate else None)


WINO = dict(options=[("SR_CONV_WINO", 2)], WINO4_MODE=0)
W64 = (1, 64, 16, 32, 64)
PW_DIRECT = dict(PW_TILED="0")
PW_TILED = dict(PW_TILED="1")
DIRECT = [("SR_CONV_WINO", 0)]


def _cases():
    """(case id, _setup arguments, the call)"""
    def conv(cid, setup, shape, **kw):
        setup = dict(setup)
        return cid, setup.pop("options", []), setup, lambda: _conv2d(shape, **kw)

    def wino(cid, shape, options=(), **kw):
        return conv(cid, dict(WINO, options=WINO["options"] + list(options)), shape, **kw)
    yield wino("wino/nt2", W64, [("SR_WINO_NT", 2)])
    yield wino("wino/nt1", W64, [("SR_WINO_NT", 1)])
    yield wino("wino/co32", (1, 64, 16, 32, 32))
    yield wino("wino/out_offset", W64, out_offset=1)
    yield wino("wino/in_offset", W64, in_offset=1)
    yield wino("wino/splitk", (1, 128, 15, 20, 128), [("SR_WINO_KSPLIT", 2)])
    yield wino("wino/split_bf16", W64, [("SR_WINO_SPLIT", "bf16"), ("SR_WINO_NT", 2)])
    yield wino("wino/split_f16", W64, [("SR_WINO_SPLIT", "f16"), ("SR_WINO_NT", 1)])
    # the training path: no split-K workspace, vector epilogue
    def train(stride):
        return lambda: autograd_ops._conv_raw(_map(*W64[:4]), torch.zeros(64, 64, 3, 3, device=DEV), torch.zeros(64, device=DEV),
                                              stride)
    yield "wino/train", WINO["options"], {}, train(1)
    yield "direct/train", DIRECT, {}, train(2)
    for form in (1, 2, 3):
        for res in (False, True):
            yield conv(f"wino4/form{form}" + "+res" * res, dict(options=[("SR_CONV_WINO", 2)], WINO4_MODE=2, WINO4_VARIANT=form),
                       (1, 16, 16, 32, 64), res=res)
    yield conv("pw/plain", PW_DIRECT, W64, k=1)
    yield conv("pw/gate", PW_DIRECT, W64, k=1, gate=True)
    for nt in (1, 2, 4):
        yield conv(f"pw/nt{nt}", dict(PW_DIRECT, options=[("SR_PW_NT", nt)]), W64, k=1)
    yield conv("pw/ks2", dict(PW_DIRECT, options=[("SR_PW_NT", 2), ("SR_PW_KS", 2)]), (1, 128, 16, 32, 64), k=1)
    yield conv("pw/co160", PW_DIRECT, (1, 64, 16, 32, 160), k=1, res=True)
    # a 2 x 15 x 20 map on the implicit-GEMM kernel: handed over as one 8-wide strip of 600 pixels
    yield conv("pw/strip", dict(options=DIRECT, USE_PW_1X1=False), (2, 64, 15, 20, 64), k=1)
    for cfg in range(4):
        yield conv(f"pt/cfg{cfg}", dict(PW_TILED, options=[("SR_PT_CFG", cfg), ("SR_PT_KS", 1)]), W64, k=1)
        yield conv(f"pt/cfg{cfg}ks2", dict(PW_TILED, options=[("SR_PT_CFG", cfg), ("SR_PT_KS", 2)]), (1, 256, 16, 32, 64), k=1)
    yield conv("pt/gate", PW_TILED, W64, k=1, gate=True)
    yield conv("pt/out_offset", dict(PW_TILED, options=[("SR_PT_KS", 2)]), (1, 256, 16, 32, 64), k=1, out_offset=1)
    direct = dict(options=DIRECT)
    yield conv("direct/3x3s2", direct, (1, 16, 16, 32, 32), s=2)
    yield conv("direct/1x1s2", direct, (1, 16, 16, 32, 32), k=1, s=2)
    yield conv("direct/replicate", direct, (1, 16, 16, 32, 32), mode="replicate")
    yield conv("direct/tf_same", direct, (1, 16, 16, 32, 32), s=2, tf_same=True)
    yield conv("direct/cin6", direct, (1, 6, 16, 32, 32))
    yield conv("direct/in_offset", direct, (1, 16, 16, 32, 32), in_offset=1)
    for tile in (1, 2, 11, 12):
        yield conv(f"direct/tile{tile}", dict(options=DIRECT + [("SR_CONV_TILE", tile)]), (1, 16, 16, 32, 64))
    yield conv("direct/s2_splitk", direct, (1, 256, 30, 40, 384), s=2)
    yield "fixed/stem7x7", [], {}, lambda: ops.stem7x7(torch.zeros(1, 3, 32, 64, device=DEV),
                                                       nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False).to(DEV))
    yield "fixed/conv1x1_stats", [], {}, lambda: ops.conv1x1_stats(_map(1, 64, 8, 16), _conv(64, 128, 1))
    yield "fixed/conv3x3_c16", [], {}, lambda: ops.conv3x3_c16(_map(1, 128, 8, 16), _conv(128, 16))


# what the fixture's kernel names have to cover, as shell-style patterns (the recorder asserts it)
COVERED = ["sr_wino_kernel<2, true, true>", "sr_wino_kernel<1, true, true>", "sr_wino_kernel<?, true, false>",
           "sr_wino_kernel<?, false, false>", "sr_wino_split_kernel<2, 1>", "sr_wino_split_kernel<1, 2>", "sr_wino4_kernel",
           "sr_wino4ws_kernel", "sr_pw_kernel<1, 1, false>", "sr_pw_kernel<2, 1, false>", "sr_pw_kernel<4, 1, false>",
           "sr_pw_kernel<2, 2, false>", "sr_pw_kernel<*, true>", "sr_pw_tiled_kernel<64x128, ks 1, false>",
           "sr_pw_tiled_kernel<128x160, ks 1, false>", "sr_pw_tiled_kernel<128x64, ks 1, false>",
           "sr_pw_tiled_kernel<64x64, ks 1, false>", "sr_pw_tiled_kernel<64x128, ks 2, false>",
           "sr_pw_tiled_kernel<128x160, ks 2, false>", "sr_pw_tiled_kernel<128x64, ks 2, false>",
           "sr_pw_tiled_kernel<64x64, ks 2, false>", "sr_pw_tiled_kernel<*, true>", "sr_conv_kernel<3, 2, *, true>",
           "sr_conv_kernel<1, 2, *", "sr_conv_kernel<1, 1, *", "sr_conv_kernel<3, 1, 1, 1, 32, true>",
           "sr_conv_kernel<3, 1, 1, 1, 8, true>", "sr_conv_kernel<3, 1, *, false>", "sr_stem_kernel", "sr_conv1x1_stats_kernel",
           "sr_t16_kernel"]
CASE_IDS = [c[0] for c in _cases()]


def run(cid):
    """The PROFILE records of case `cid` as [[kernel name, algorithmic FLOPs, shape, executed FLOPs or None], ...]."""
    (options, attrs, call), = [c[1:] for c in _cases() if c[0] == cid]
    prof = []
    with _setup(options, **attrs), torch.no_grad():
        ops.PROFILE = prof
        try:
            call()
        finally:
            ops.PROFILE = None
    torch.cuda.synchronize()
    return [[name, flops, list(shape), executed] for name, flops, _, _, shape, executed in prof]


def device_cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count
