"""Host-side logic of the cost-volume managers and of the whole DepthModel on CPU: the C-ABI library is replaced by a stub that checks every call
against the ctypes signature table (argument count and kinds) and returns success, so the Python control flow --
argument packing, output allocation, mask handling, the autograd seams and their bookkeeping -- runs without a GPU.
No numerics here: the kernels themselves are covered by the `-m gpu` tests."""
import contextlib
import gzip
import json
import os
import ctypes
import weakref

import pytest
import torch

from simplerecon_amd import _lib, synthetic
from simplerecon_amd import cost_volume as cv

B, K, C, H, W, D = 2, 3, 16, 8, 12, 4


_BYREF = type(ctypes.byref(ctypes.c_int()))


def make_stub(monkeypatch):
    class Calls(list):
        prefer_wino = False
        prefer_wino4 = 0     # the F(4x4) kernel form sr_conv_prefers_wino4 answers
        prefer16 = 0         # sr_conv16_prefers: 0 / 1, or the set of shapes (its arguments) it answers 1 for
        prefer16_wgrad = 0   # sr_conv16_wgrad_prefers
    calls = Calls()
    calls.args = []          # (name, arguments) of every stubbed call
    calls.option_sets = []   # (id, value) of every sr_option_set, forwarded to the real library
    calls.rc = {}            # entry point -> the code it returns (default 0: success)
    calls.hooks = {}         # entry point -> callable(*args) run inside the stubbed call

    class Stream:
        cuda_stream = 0

    class Event:   # (torch.cuda.Event without a GPU: the PROFILE records and the pack fences only keep them)
        def __init__(self, **kw):
            pass

        def record(self, *a):
            pass

        def query(self):
            return True

    class Fn:
        def __init__(self, name):
            self.name = name

        def __call__(self, *args):
            res, argtypes = _lib.SIGNATURES[self.name]
            assert len(args) == len(argtypes), (self.name, len(args), len(argtypes))
            for v, t in zip(args, argtypes):
                if t is ctypes.c_void_p:
                    assert v is None or isinstance(v, (ctypes.c_void_p, int, _BYREF)), (self.name, type(v))
                elif t is ctypes.c_float:
                    assert isinstance(v, (float, ctypes.c_float)), (self.name, type(v))
                else:
                    assert isinstance(v, int), (self.name, type(v), v)
            calls.append(self.name)
            calls.args.append((self.name, args))
            if self.name in calls.hooks:
                calls.hooks[self.name](*args)
            if self.name == "sr_conv_prefers_wino":
                return int(calls.prefer_wino)
            if self.name == "sr_conv_prefers_wino4":
                return calls.prefer_wino4
            if self.name == "sr_conv16_prefers":
                return int(args in calls.prefer16) if isinstance(calls.prefer16, (set, frozenset)) else calls.prefer16
            if self.name == "sr_conv16_wgrad_prefers":
                return calls.prefer16_wgrad
            if self.name.endswith("_supported"):
                return 1
            if self.name == "sr_last_launch":
                # (kernel name, executed FLOPs) through the out-pointers: the launcher call before it, nothing executed
                args[0]._obj.value = b"stub:" + calls[-2].encode()
                args[2]._obj.value = -1.0
            if res is ctypes.c_char_p:
                return b"stub_kernel"
            return 4096 if res is ctypes.c_size_t else calls.rc.get(self.name, 0)

    real = _lib.lib()   # (the option table is host-only code: those calls go to the real library, GPU or not)

    def option_set(oid, value, previous):
        calls.option_sets.append((oid, value))
        return real.sr_option_set(oid, value, previous)

    class Lib:
        def __getattr__(self, name):
            if name == "sr_option_set":
                return option_set
            return getattr(real, name) if name.startswith("sr_option_") else Fn(name)

    from simplerecon_amd import ops
    monkeypatch.setattr(ops, "_SHAPE_QUERIES", {})   # per-shape answers of the (stubbed) library are cached per process
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    monkeypatch.setattr(_lib, "require_device_f32", lambda *a, **k: None)
    monkeypatch.setattr(_lib, "stream_ptr", lambda dev=None: ctypes.c_void_p(0))
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "current_stream", lambda d=None: Stream())
    monkeypatch.setattr(torch.cuda, "Event", Event)
    return calls


@pytest.fixture
def stub(monkeypatch):
    return make_stub(monkeypatch)


@pytest.mark.parametrize("cls,kw,fwd", [(cv.CostVolumeManager, {}, "sr_dot_volume_fwd"),
                                        (cv.FeatureVolumeManager, dict(num_source_views=K), "sr_mlp_volume_fwd"),
                                        (cv.FastFeatureVolumeManager, dict(num_source_views=K), "sr_mlp_volume_fwd")])
def test_inference_paths(stub, cls, kw, fwd):
    inp = synthetic.cost_volume_inputs(B, K, C, H, W, seed=1)
    mgr = cls(H, W, num_depth_bins=D, **kw)
    for return_mask in (False, True):
        del stub[:]
        with torch.inference_mode():
            vol, lowest, planes, mask = mgr(return_mask=return_mask, **inp)
        assert vol.shape == (B, D, H, W) and lowest.shape == (B, H, W) and planes.shape == (B, D, H, W)
        # the dot model ignores return_mask (reference cost_volume.py:286, 335)
        assert (mask is None) == (not return_mask or cls is cv.CostVolumeManager)
        assert mask is None or mask.dtype == torch.bool
        assert stub[-1] == fwd
    # grad mode on: like any nn.Module, a manager whose parameters require grad builds an autograd graph (the MLP
    # managers -- reference train.py trains the matching MLP); with no parameters and constant features it does not
    assert mgr(**inp)[0].requires_grad == (cls is not cv.CostVolumeManager)
    for p_ in mgr.parameters():
        p_.requires_grad_(False)
    assert not mgr(**inp)[0].requires_grad
    # empty batch: nothing is launched
    empty = {k: (v[:0] if v.dim() > 0 and v.shape[0] == B and k not in ("min_depth", "max_depth") else v)
             for k, v in inp.items()}
    del stub[:]
    with torch.inference_mode():
        vol = mgr(**empty)[0]
    assert vol.shape == (0, D, H, W) and not [c for c in stub if c.endswith("_fwd")]


def _reserve_arg(stub):
    name, args = [c for c in stub.args if c[0] == "sr_mlp_volume_fwd"][-1]
    argtypes = _lib.SIGNATURES[name][1]
    assert argtypes[-4:] == [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    return args[-4]   # reserve_cus, just before workspace, workspace_bytes, stream


@pytest.mark.parametrize("cls", [cv.FeatureVolumeManager, cv.FastFeatureVolumeManager])
def test_cu_reserve_is_an_argument_of_the_call(stub, cls):
    """The MLP sweep's CU reserve reaches sr_mlp_volume_fwd as a call argument (0 by default) and touches no library option."""
    inp = synthetic.cost_volume_inputs(B, K, C, H, W, seed=1)
    mgr = cls(H, W, num_depth_bins=D, num_source_views=K)
    with torch.inference_mode():
        mgr(**inp)
        assert _reserve_arg(stub) == 0
        mgr(reserve_cus=32, **inp)
        assert _reserve_arg(stub) == 32
        mgr(**inp)
        assert _reserve_arg(stub) == 0
    assert stub.option_sets == []


def test_autograd_seams(stub):
    inp = synthetic.cost_volume_inputs(B, K, C, H, W, seed=1)
    # dot model: differentiable w.r.t. the features out of the box
    dot = cv.CostVolumeManager(H, W, num_depth_bins=D)
    cur, src = inp["cur_feats"].clone().requires_grad_(), inp["src_feats"].clone().requires_grad_()
    vol, lowest, _, _ = dot(**dict(inp, cur_feats=cur, src_feats=src))
    assert vol.requires_grad and not lowest.requires_grad
    vol.sum().backward()
    assert stub[-2:] == ["sr_volume_prepare", "sr_dot_volume_bwd"] and cur.grad.shape == cur.shape
    assert src.grad.shape == src.shape
    with pytest.raises(NotImplementedError):
        dot(**dict(inp, src_Ks=inp["src_Ks"].clone().requires_grad_()))
    # MLP model: differentiable out of the box (a swapped-in manager trains under train.py); opting out refuses
    hero = cv.FeatureVolumeManager(H, W, num_depth_bins=D, num_source_views=K)
    hero.differentiable = False
    with pytest.raises(NotImplementedError):
        hero(**dict(inp, cur_feats=cur))
    del hero.differentiable
    assert hero.differentiable
    cur.grad = None
    vol, lowest, _, mask = hero(**dict(inp, cur_feats=cur), return_mask=True)
    assert vol.requires_grad and not lowest.requires_grad and mask.dtype == torch.bool and not mask.requires_grad
    vol.sum().backward()
    assert stub[-2:] == ["sr_volume_prepare", "sr_mlp_volume_bwd"]
    assert cur.grad is not None and all(p.grad is not None and p.grad.shape == p.shape for p in hero.mlp.parameters())
    with torch.no_grad():
        assert not hero(**dict(inp, cur_feats=cur))[0].requires_grad


@pytest.mark.parametrize("prefer_wino", [False, True])
@pytest.mark.parametrize("fvt", ["mlp_feature_volume", "simple_cost_volume"])
def test_whole_model_control_flow(stub, prefer_wino, fvt):
    """DepthModel.forward end to end through the stub: every stage reaches its entry point with a well-formed call and
    the output dict has the reference's keys and shapes (depth_model.py:388-405)."""
    from simplerecon_amd import depth_model as dm
    stub.prefer_wino = prefer_wino
    b, k, h, w, d = 1, 2, 96, 128, 8
    opts = dm.default_options(image_width=w, image_height=h, model_num_views=k + 1, matching_num_depth_bins=d,
                              feature_volume_type=fvt)
    model = dm.DepthModel(opts).eval()
    inp = synthetic.cost_volume_inputs(b, k, 16, h // 4, w // 4, seed=2)
    eye = torch.eye(4).expand(b, 4, 4).contiguous()
    cur = {"image_b3hw": torch.randn(b, 3, h, w), "invK_s1_b44": inp["cur_invK"], "cam_T_world_b44": eye,
           "world_T_cam_b44": eye}
    src = {"image_b3hw": torch.randn(b, k, 3, h, w), "K_s1_b44": inp["src_Ks"],
           "cam_T_world_b44": inp["src_extrinsics"], "world_T_cam_b44": inp["src_poses"]}
    with torch.inference_mode():
        out = model("test", cur, src, return_mask=True)
    assert stub.option_sets == []   # the forward changes no process-wide library option
    for i in range(4):
        assert out[f"log_depth_pred_s{i}_b1hw"].shape == (b, 1, (h // 2) >> i, (w // 2) >> i)
        assert out[f"depth_pred_s{i}_b1hw"].shape == (b, 1, (h // 2) >> i, (w // 2) >> i)
    assert out["lowest_cost_bhw"].shape == (b, h // 4, w // 4)
    assert (out["overall_mask_bhw"] is None) == (fvt == "simple_cost_volume")
    seen = set(stub)
    sweep = "sr_mlp_volume_fwd" if fvt == "mlp_feature_volume" else "sr_dot_volume_fwd"
    for name in (sweep, "sr_stem7x7_fwd", "sr_maxblurpool_nhwc_fwd", "sr_conv1x1_stats_nhwc_fwd", "sr_conv3x3_c16_nhwc_fwd",
                 "sr_conv2d_padded_nhwc_fwd", "sr_dwconv3x3_nhwc_fwd", "sr_se_gate2_fwd", "sr_pw_conv_nhwc_fwd", "sr_add_nhwc_fwd",
                 "sr_upsample2x_nhwc_fwd", "sr_exp_fwd",
                 "sr_conv3x3_wino_splitk_nhwc_fwd" if prefer_wino else "sr_conv2d_splitk_nhwc_fwd"):
        assert name in seen, name
    assert stub.count("sr_dwconv3x3_nhwc_fwd") == 30 and stub.count("sr_upsample2x_nhwc_fwd") == 16


def test_sweep_reserve_rule():
    """DepthModel leaves `sweep_reserved_cus` CUs to the image-prior encoder while that still runs on its side stream (a
    pending pyramid), for metadata-MLP sweeps of up to `sweep_reserve_max_points` (pixel, plane) points; otherwise none."""
    from simplerecon_amd import depth_model as dm
    model = dm.DepthModel(dm.default_options(image_width=640, image_height=480, matching_num_depth_bins=64))
    assert isinstance(model.cost_volume, cv.FeatureVolumeManager) and model.cost_volume.num_depth_bins == 64
    feats = [torch.empty(0)] * 5
    pending = dm.PendingPyramid(None, feats)
    one, eight = torch.empty(1, 16, 120, 160), torch.empty(8, 16, 120, 160)
    assert model.sweep_reserved_cus == 32 and model.sweep_reserve_max_points == 5_000_000
    assert model._sweep_reserve(pending, one) == 32
    assert model._sweep_reserve(pending, eight) == 0
    assert model._sweep_reserve(feats, one) == 0
    model.cost_volume = cv.CostVolumeManager(120, 160, num_depth_bins=64)
    assert model._sweep_reserve(pending, one) == 0


def test_lazy_levels():
    """networks.LazyLevels, the one lazy sequence of the inference schedule: a callable item is resolved on first use and
    kept; slices and sums share the items and resolve nothing, nor do peek() and unresolved(); indices are a list's."""
    from simplerecon_amd import depth_model as dm
    from simplerecon_amd.networks import LazyLevels
    t = [torch.full((1,), float(i)) for i in range(4)]
    calls = []

    def later(i, known=True):
        def resolve():
            calls.append(i)
            return t[i]
        if known:
            resolve.tensor = t[i]
        return resolve
    levels = LazyLevels([t[0], later(1), later(2), later(3, known=False)])
    assert len(levels) == 4 and LazyLevels.of(levels) is levels and len(LazyLevels.of(t)) == 4
    peek = levels.peek()
    assert all(a is b for a, b in zip(peek, t[:3])) and peek[3] is None
    tail, both = levels[1:], [t[0]] + levels[2:] + [t[1]]
    assert isinstance(tail, LazyLevels) and isinstance(both, LazyLevels) and (len(tail), len(both)) == (3, 4)
    assert [levels.unresolved(i) for i in range(4)] == [False, True, True, True] and tail.unresolved(-1) and calls == []
    assert tail[1] is t[2] and calls == [2]              # resolved through the slice ...
    assert levels[2] is t[2] and both[1] is t[2] and calls == [2]   # ... once, for every view of the same items
    assert not levels.unresolved(2) and levels.unresolved(1) and levels.peek()[2] is t[2]
    assert levels[-1] is t[3] and levels[-4] is t[0] and calls == [2, 3]
    assert [x is y for x, y in zip(levels, t)] == [True] * 4 and calls == [2, 3, 1]   # iterating resolves the rest, in order
    for bad in (4, -5):
        with pytest.raises(IndexError):
            levels[bad]
        with pytest.raises(IndexError):
            levels.unresolved(bad)
    with pytest.raises(TypeError):
        levels["0"]
    # a pending pyramid's levels are such a sequence: reference-style slicing works and joins nothing
    feats = [torch.empty(0)] * 5
    rest = dm.PendingPyramid(None, feats).levels_from(1)[1:]
    assert isinstance(rest, LazyLevels) and len(rest) == 3 and all(rest.unresolved(i) for i in range(3))
    assert all(p is f for p, f in zip(rest.peek(), feats))


def test_autocast_region_upcasts_half_features(stub):
    """Reference training runs under 16-bit autocast (options.py:100-101): inside an autocast region half-precision
    matching features are upcast to fp32 for the HIP kernels and the gradients come back in the caller's dtype."""
    inp = synthetic.cost_volume_inputs(B, K, C, H, W, seed=1)
    dot = cv.CostVolumeManager(H, W, num_depth_bins=D)
    cur = inp["cur_feats"].bfloat16().requires_grad_()
    src = inp["src_feats"].bfloat16().requires_grad_()
    with torch.autocast("cpu", dtype=torch.bfloat16):
        vol = dot(**dict(inp, cur_feats=cur, src_feats=src))[0]
    assert vol.dtype == torch.float32 and vol.requires_grad
    vol.sum().backward()
    assert cur.grad.dtype == torch.bfloat16 and src.grad.dtype == torch.bfloat16
    assert stub[-1] == "sr_dot_volume_bwd"


def test_packed_weight_cache_key_follows_the_parameters():
    """ops._state_key decides whether a cached packed weight is still valid: it must change when a parameter is updated in
    place (optimizer step, load_state_dict), replaced by a new tensor (module.to(...), re-assignment), or when the folded
    BatchNorm's statistics move -- and must not change otherwise."""
    from torch import nn

    from simplerecon_amd import ops
    conv, bn = nn.Conv2d(8, 16, 3, padding=1), nn.BatchNorm2d(16)
    k0, k0_bn = ops._state_key(conv, None), ops._state_key(conv, bn)
    assert ops._state_key(conv, None) == k0 and ops._state_key(conv, bn) == k0_bn and k0 != k0_bn
    with torch.no_grad():
        conv.weight.mul_(2.0)                                   # in-place update: version bump
    k1 = ops._state_key(conv, None)
    assert k1 != k0
    conv.load_state_dict({k: v.clone() for k, v in conv.state_dict().items()})   # copy_ into the same storage
    k2 = ops._state_key(conv, None)
    assert k2 != k1
    conv.weight = nn.Parameter(conv.weight.detach().clone())    # a new tensor object
    k3 = ops._state_key(conv, None)
    assert k3 != k2
    conv.bias = None
    assert ops._state_key(conv, None) != k3 and len(ops._state_key(conv, None)) == 2
    kb = ops._state_key(conv, bn)
    bn.running_var.add_(1.0)
    assert ops._state_key(conv, bn) != kb
    plain = nn.BatchNorm2d(16, affine=False)
    assert len(ops._state_key(conv, plain)) == 3               # weight + the two running statistics


def test_per_shape_library_answers_are_asked_once(stub):
    from simplerecon_amd import ops
    lib = _lib.lib()
    assert ops._shape_query(lib, "sr_conv_prefers_wino", 1, 8, 16, 16, 32, 3, 1) == 0
    n = len(stub)
    stub.prefer_wino = True     # the library's answer is a pure function of the shape: the cached one is returned
    assert ops._shape_query(lib, "sr_conv_prefers_wino", 1, 8, 16, 16, 32, 3, 1) == 0 and len(stub) == n
    assert ops._shape_query(lib, "sr_conv_prefers_wino", 2, 8, 16, 16, 32, 3, 1) == 1 and len(stub) == n + 1


def test_split_precision_switch_repacks_the_cached_winograd_weight(stub, monkeypatch, sr_option):
    """SR_WINO_SPLIT (the fenced split-precision Winograd variant) changes what a packed weight CONTAINS (16-bit pieces in the
    fp32 layout's buffer): the cache must re-pack when the switch changes and hit otherwise; off-values mean the fp32 path."""
    from torch import nn

    from simplerecon_amd import ops
    monkeypatch.setattr(ops, "_PACKED", weakref.WeakKeyDictionary())
    conv = nn.Conv2d(16, 32, 3, padding=1)
    for off in ("", "0", "off", "fp32"):
        sr_option("SR_WINO_SPLIT", off)
        assert ops.wino_split_mode() == ""
    ops.packed_wino_weight(conv)
    n = stub.count("sr_wino_pack_weights")
    ops.packed_wino_weight(conv)
    assert stub.count("sr_wino_pack_weights") == n            # cache hit
    sr_option("SR_WINO_SPLIT", "f16")
    assert ops.wino_split_mode() == "f16"
    ops.packed_wino_weight(conv)
    assert stub.count("sr_wino_pack_weights") == n + 1        # re-packed as 16-bit pieces
    ops.packed_wino_weight(conv)
    assert stub.count("sr_wino_pack_weights") == n + 1
    sr_option("SR_WINO_SPLIT", "bf16")
    ops.packed_wino_weight(conv)
    assert stub.count("sr_wino_pack_weights") == n + 2
    sr_option("SR_WINO_SPLIT", "0")
    ops.packed_wino_weight(conv)
    assert stub.count("sr_wino_pack_weights") == n + 3        # and back to fp32 fragments


def test_a_split_mode_set_during_the_pack_does_not_reach_the_launch(stub, monkeypatch, sr_option):
    """The Winograd split format is read once per call and carried from the pack to the launch as a value (the C ABI's
    `split_format`): here another thread sets SR_WINO_SPLIT to another mode from INSIDE sr_wino_pack_weights, during an
    ops.conv2d and during an autograd_ops._ConvBiasAct forward.  The launch that follows carries the format the pack carried;
    the next call, under the mode now set, packs again in that mode (the cache keys on the format); and the thread that
    set the mode was never kept waiting.  This replaces test_split_option_listeners_run_under_the_split_guard of
    tests/test_abi.py, which tested the lock that used to stand for the property.  Before the format became an argument the
    training-path half failed -- _conv_raw held no lock and the launcher read the option table again after the pack, so the
    fp16-piece weights met the bf16 kernel -- and in the conv2d half the setting thread hung on the lock instead."""
    import threading

    from torch import nn

    from simplerecon_amd import autograd_ops, ops
    monkeypatch.setattr(ops, "_PACKED", weakref.WeakKeyDictionary())
    stub.prefer_wino = True
    pack_fmt = _lib.SIGNATURES["sr_wino_pack_weights"][1].index(ctypes.c_int, 3)                # behind Cout, Cin
    launch_fmt = _lib.SIGNATURES["sr_conv3x3_wino_splitk_nhwc_fwd"][1].index(ctypes.c_float) + 1   # behind leaky_slope
    assert pack_fmt == 3 and launch_fmt == 17
    kept_waiting = []

    def set_another_mode(*args):
        t = threading.Thread(target=_lib.set_option, args=("SR_WINO_SPLIT", {0: 2, 1: 2, 2: 1}[args[pack_fmt]]))
        t.start()
        t.join(10)   # (returns at once unless set_option blocks)
        kept_waiting.append(t.is_alive())
    stub.hooks["sr_wino_pack_weights"] = set_another_mode

    def formats():
        """[format of each pack, format of each Winograd launch] since the last look"""
        got = [[a[pack_fmt] for n, a in stub.args if n == "sr_wino_pack_weights"],
               [a[launch_fmt] for n, a in stub.args if n == "sr_conv3x3_wino_splitk_nhwc_fwd"]]
        del stub[:], stub.args[:]
        return got
    conv = nn.Conv2d(16, 32, 3, padding=1)
    x = torch.zeros(1, 16, 8, 16).contiguous(memory_format=torch.channels_last)
    sr_option("SR_WINO_SPLIT", "f16")
    del stub[:], stub.args[:]
    with torch.no_grad():
        ops.conv2d(x, conv)
        assert formats() == [[2], [2]] and _lib.get_option("SR_WINO_SPLIT") == 1   # packed as f16 pieces, launched as such
        ops.conv2d(x, conv)
        assert formats() == [[1], [1]] and _lib.get_option("SR_WINO_SPLIT") == 2   # the mode set meanwhile: packed again
        ops.conv2d(x, conv)
        assert formats() == [[2], [2]]   # (the cache holds one format per layer)
        del stub.hooks["sr_wino_pack_weights"]
        ops.conv2d(x, conv)
        assert formats() == [[1], [1]]
        ops.conv2d(x, conv)
        assert formats() == [[], [1]]    # nothing set in between: a cache hit
    stub.hooks["sr_wino_pack_weights"] = set_another_mode
    w, b = conv.weight.detach().requires_grad_(), conv.bias.detach()
    _lib.set_option("SR_WINO_SPLIT", "f16")
    autograd_ops._ConvBiasAct.apply(x, w, b, None, 1, 0.1, None)
    assert formats() == [[2], [2]] and _lib.get_option("SR_WINO_SPLIT") == 1
    autograd_ops._ConvBiasAct.apply(x, w, b, None, 1, 0.1, None)
    assert formats() == [[1], [1]] and _lib.get_option("SR_WINO_SPLIT") == 2
    _lib.set_option("SR_WINO_SPLIT", 0)
    autograd_ops._ConvBiasAct.apply(x, w, b, None, 1, 0.1, None)
    assert formats() == [[0], [0]]
    assert kept_waiting == [False] * 6


def _cached_entry_points():
    """name -> (module, eval-mode BatchNorm folded into it or None, one call that uses the cached payload) for each ops entry
    point with a packed-weight cache entry."""
    from torch import nn

    from simplerecon_amd import ops
    nhwc = lambda *shape: torch.zeros(*shape).contiguous(memory_format=torch.channels_last)
    bn = lambda c: nn.BatchNorm2d(c).eval()
    conv3 = lambda: nn.Conv2d(8, 16, 3, padding=1)
    return {
        "direct": (conv3(), bn(16), lambda m, n: ops.packed_weight(m, n)),
        "wino": (conv3(), bn(16), lambda m, n: ops.packed_wino_weight(m, n)),
        "wino4": (conv3(), bn(16), lambda m, n: ops.packed_wino4_weight(m, n)),
        "linear": (nn.Linear(8, 16), None, lambda m, n: ops.linear(torch.zeros(4, 8), m)),
        "stem": (nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False), bn(64),
                 lambda m, n: ops.stem7x7(torch.zeros(1, 3, 16, 16), m, n)),
        "c16": (nn.Conv2d(32, 16, 3, padding=1), None, lambda m, n: ops.conv3x3_c16(nhwc(1, 32, 8, 8), m)),
        "dw": (nn.Conv2d(16, 16, 3, padding=1, groups=16, bias=False), bn(16),
               lambda m, n: ops.dwconv3x3(nhwc(1, 16, 8, 8), m, n)),
        "rgb": (nn.Conv2d(3, 24, 3, stride=2, bias=False), bn(24),
                lambda m, n: ops.rgb_stem3x3s2(torch.zeros(1, 3, 16, 16), m, n)),
    }


_CACHED = sorted(_cached_entry_points())


@pytest.mark.parametrize("name", _CACHED)
def test_packed_weights_are_cached_until_a_parameter_changes(stub, monkeypatch, name):
    """Each cached entry point packs once, hits afterwards, and re-packs after an in-place parameter update, a new
    nn.Parameter and a change of a folded BatchNorm's running statistics."""
    from torch import nn

    from simplerecon_amd import ops
    mod, bn, use = _cached_entry_points()[name]
    builds, cached = [], ops._cached
    monkeypatch.setattr(ops, "_cached", lambda m, tag, key, build, *args: cached(
        m, tag, key, lambda *a: (builds.append(tag), build(*a))[1], *args))

    def packs():
        with torch.no_grad():
            use(mod, bn)
            use(mod, bn)
        return len(builds)
    assert packs() == 1
    with torch.no_grad():
        mod.weight.mul_(2.0)
    assert packs() == 2
    mod.weight = nn.Parameter(mod.weight.detach().clone())
    assert packs() == 3
    if bn is not None:
        bn.running_mean.add_(1.0)
        assert packs() == 4


def test_what_the_cache_key_can_and_cannot_see():
    """The eager cache key is (version, address): in-place updates under no_grad, load_state_dict, nn.init.* and writes through
    detach() bump the version counter; writes through `.data` do not -- the documented blind spot ops.forget_packed is for."""
    from torch import nn

    from simplerecon_amd import ops
    conv = nn.Conv2d(4, 4, 3, padding=1)
    key = lambda: ops._state_key(conv, None)
    for write in (lambda: conv.weight.data.mul_(2.0), lambda: conv.weight.data.copy_(torch.ones_like(conv.weight)),
                  lambda: conv.bias.data.add_(1.0)):
        before = key()
        write()
        assert key() == before
    bumps = [lambda: conv.weight.mul_(2.0), lambda: conv.load_state_dict({k: v.clone() for k, v in conv.state_dict().items()}),
             lambda: nn.init.ones_(conv.weight), lambda: conv.weight.detach().mul_(0.5), lambda: conv.bias.detach().zero_()]
    for write in bumps:
        before = key()
        with torch.no_grad():
            write()
        assert key() != before


@pytest.mark.parametrize("name", _CACHED)
def test_forget_packed_makes_a_data_write_visible(stub, monkeypatch, name):
    """A `.data` write leaves the cached payload in place (the key cannot see it); after ops.forget_packed -- on the module or
    on any module above it -- the next call packs again, from the weights as they are then."""
    from torch import nn

    from simplerecon_amd import ops
    monkeypatch.setattr(ops, "_PACKED", weakref.WeakKeyDictionary())
    mod, bn, use = _cached_entry_points()[name]
    builds, cached = [], ops._cached

    def counting(m, tag, key, build, *args):
        def build_(*a):
            payload = build(*a)
            builds.append((tag, payload))
            return payload
        return cached(m, tag, key, build_, *args)
    monkeypatch.setattr(ops, "_cached", counting)

    def packs():
        with torch.no_grad():
            use(mod, bn)
            use(mod, bn)
        return len(builds)
    assert packs() == 1
    mod.weight.data.mul_(3.0)
    assert packs() == 1                                  # stale: nothing told the cache
    epoch = ops._FORGET_EPOCH
    ops.forget_packed(mod)
    assert ops._FORGET_EPOCH == epoch + 1 and mod not in ops._PACKED
    assert packs() == 2
    if bn is not None:
        bn.running_var.data.mul_(4.0)
        assert packs() == 2
        ops.forget_packed(nn.Sequential(nn.Sequential(mod), bn))   # from a root two levels up
        assert packs() == 3
    if name == "dw":    # (a payload built by torch rather than the stubbed library: its values are those of the new weights)
        w9c = builds[-1][1][0]
        scale = ops.bn_affine(bn)[0]
        assert torch.allclose(w9c, (mod.weight.detach() * scale.view(-1, 1, 1, 1)).reshape(16, 9).t())
    assert all(p is not None for p in ops.packed_payloads([mod])) and len(ops.packed_payloads([mod])) == 1
    assert ops.packed_payloads([nn.Conv2d(1, 1, 1)]) == []


def test_graph_weight_check_sees_what_changes_a_weight():
    """graph._weight_state / GraphedCallable._check_weights (the replay check of DepthModel.graphed) on the CPU: silent while
    nothing changed; raises after an in-place update, load_state_dict, a replaced parameter, a moved buffer."""
    from torch import nn

    from simplerecon_amd import graph

    def checker(model):
        g = graph.GraphedCallable.__new__(graph.GraphedCallable)
        g._weights = graph._weight_state([model])
        return g._check_weights
    model = nn.Sequential(nn.Conv2d(3, 4, 3), nn.BatchNorm2d(4), nn.Sequential(nn.Linear(4, 2)))
    assert len(graph._weight_state([model])) == 2 + 5 + 2 and len(graph._weight_state([model, model[2]])) == 9
    check = checker(model)
    check()
    check()
    with torch.no_grad():
        model[0].weight.mul_(2.0)
    with pytest.raises(graph.StaleGraphError, match="capture") as err:
        check()
    assert "`Sequential.0.weight`" in str(err.value)     # which module's weight, not only its local name
    check = checker(model)
    model[2][0].bias.detach().zero_()
    with pytest.raises(graph.StaleGraphError, match=r"`Sequential\.2\.0\.bias`"):
        check()
    for change in (lambda: model.load_state_dict({k: v.clone() for k, v in model.state_dict().items()}),
                   lambda: setattr(model[2][0], "weight", nn.Parameter(model[2][0].weight.detach().clone())),
                   lambda: model[1].running_mean.add_(1.0),
                   lambda: model.double()):
        check = checker(model)
        check()
        change()
        with pytest.raises(graph.StaleGraphError):
            check()
    check = checker(model)
    model[0].weight.data.mul_(2.0)       # the blind spot: ops.forget_packed() is what invalidates a graph then
    check()


@pytest.mark.parametrize("name", _CACHED)
def test_packed_weights_are_fenced_for_other_streams(stub, monkeypatch, name):
    """A payload packed on stream A is waited for once by a use on stream B while the pack has not completed, never by a use
    on A; a completed pack is not waited for again; while a graph is captured nothing is recorded or awaited."""
    class Stream:
        def __init__(self, handle):
            self.cuda_stream, self.waits = handle, []

        def wait_event(self, ev):
            self.waits.append(ev)

    events = []

    class Event:
        def __init__(self, **kw):
            self.stream, self.done, self.queries = None, False, 0
            events.append(self)

        def record(self, stream=None):
            self.stream = stream

        def query(self):
            self.queries += 1
            return self.done

    a, b = Stream(1), Stream(2)
    now = {"stream": a, "capturing": False}
    monkeypatch.setattr(torch.cuda, "current_stream", lambda d=None: now["stream"])
    monkeypatch.setattr(torch.cuda, "Event", Event)
    monkeypatch.setattr(_lib, "cuda_available", lambda: True)
    monkeypatch.setattr(_lib, "capturing", lambda: now["capturing"])
    mod, bn, use = _cached_entry_points()[name]

    def run(stream, capturing=False):
        now["stream"], now["capturing"] = stream, capturing
        with torch.no_grad():
            use(mod, bn)
    run(a)
    assert len(events) == 1 and events[0].stream is a
    ev = events[0]
    run(a)
    assert a.waits == []
    queries = ev.queries
    run(b, capturing=True)
    assert b.waits == [] and ev.queries == queries and len(events) == 1
    run(b)
    assert b.waits == [ev]
    ev.done = True
    run(b)
    queries = ev.queries
    run(b)
    assert b.waits == [ev] and ev.queries == queries
    with torch.no_grad():
        mod.weight.mul_(2.0)
    run(a, capturing=True)   # a re-pack inside a capture
    run(b)
    assert len(events) == 1 and b.waits == [ev] and a.waits == []


def test_fenced_workloads_label_their_arithmetic():
    """The split-precision workloads are separate registry entries whose bench line says what they compute with; the default
    workload is the fp32 one."""
    import bench_workloads as bw
    assert bw.DEFAULT == "hero_cfg3" and bw.HeroCfg3.dtype == "f32"
    for name in ("hero_cfg3_bf16x3", "hero_cfg3_f16x3", "hero_cfg3_bf16x3_convs", "hero_cfg3_f16x3_convs"):
        assert name in bw.WORKLOADS


def test_split_precision_context_manager_sets_and_restores_the_switches(sr_option):
    """The context manager drives the library's option table (no os.environ mutation: ADVICE r04) and nests."""
    from simplerecon_amd import experimental, ops
    env_before = dict(os.environ)
    sr_option("SR_MLP_SPLIT", 0)
    sr_option("SR_WINO_SPLIT", "bf16")
    mlp = lambda: _lib.split_mode_name("SR_MLP_SPLIT")
    with experimental.split_precision("f16"):
        assert mlp() == "f16" and ops.wino_split_mode() == "f16"
        with experimental.split_precision("bf16", convs=False):
            assert mlp() == "bf16" and ops.wino_split_mode() == "f16"
        assert mlp() == "f16"
    assert mlp() == "" and ops.wino_split_mode() == "bf16"
    assert dict(os.environ) == env_before
    with pytest.raises(ValueError):
        with experimental.split_precision("int8"):
            pass


def test_batchnorm_layer_cache_sees_replacements_deep_in_the_tree():
    """the cached list of batch-norm layers behind `any_batchnorm_training` must be rebuilt when a layer is
    swapped ANYWHERE in the tree (SyncBatchNorm conversion, fusion), and must recognise every `_BatchNorm` flavour."""
    from torch import nn
    from simplerecon_amd import autograd_ops as A
    m = nn.Sequential(nn.Sequential(nn.Conv2d(3, 3, 1), nn.BatchNorm2d(3)), nn.ReLU()).eval()
    assert not A.any_batchnorm_training(m)
    m[0][1] = nn.BatchNorm2d(3)                      # a fresh layer (training mode) two levels down
    assert A.any_batchnorm_training(m)
    m.eval()
    assert not A.any_batchnorm_training(m)
    m[0][1] = nn.SyncBatchNorm(3)                    # not an nn.BatchNorm2d, still batch statistics
    assert A.any_batchnorm_training(m)
    m[0][1].eval()
    assert not A.any_batchnorm_training(m)
    m[0][1].train()                                  # a flag flipped on the leaf only
    assert A.any_batchnorm_training(m)


def test_batchnorm_layer_cache_sees_direct_mutations_of_modules():
    """torch's registration hook does not fire for direct `_modules` mutations (del m.bn, ModuleList.__delitem__,
    fx / quantisation swaps); a cached layer that no longer sits where it was found invalidates the cache."""
    from torch import nn
    from simplerecon_amd import autograd_ops as A
    inner = nn.Sequential(nn.BatchNorm2d(3))
    m = nn.Sequential(nn.Conv2d(3, 3, 1), inner).eval()
    assert not A.any_batchnorm_training(m)
    fresh = nn.BatchNorm2d(3)                        # training mode
    inner._modules["0"] = fresh                      # swapped in behind the hook's back
    assert A.any_batchnorm_training(m)
    del inner._modules["0"]                          # and removed the same way
    assert not A.any_batchnorm_training(m)
    bn = nn.BatchNorm2d(2)                           # a batch-norm layer as the root of the query
    assert A.any_batchnorm_training(bn)
    assert not A.any_batchnorm_training(bn.eval())


# ---- ops.conv2d dispatch, pinned --------------------------------------------------------------------------------------
# Which library entry points ops.conv2d calls (in order, with every non-pointer argument), and the ops.PROFILE records it
# appends, over a grid of layer shapes, tensor layouts and library answers -- including SR_ERR_UNSUPPORTED (2) injected on
# each entry point a case falls back from, and a hard error (1) on the first one.  Recorded in
# tests/golden/conv2d_dispatch.json.gz; a case that raises pins its exception instead of its records.
_GOLDEN_DISPATCH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv2d_dispatch.json.gz")


def _dispatch_cases():
    answers = [(False, 0, ""), (True, 0, ""), (True, 1, ""), (True, 3, ""), (True, 0, "f16"), (True, 0, "bf16")]
    for k in (1, 3):
        for s in (1, 2):
            for pad in ("zeros", "replicate", "tf_same"):
                pw = k == 1 and s == 1 and pad != "replicate"   # cases the pointwise kernels may take
                for aligned in (True, False):
                    for out_slice in (False, True):
                        for res in (False, True):
                            for gate in ((False, True) if k == 1 else (False,)):
                                for wino, w4, split in (answers if (k, s) == (3, 1) else answers[:1]):
                                    for tiled in ((False, True) if pw else (False,)):
                                        for pw1x1 in ((True, False) if pw else (True,)):
                                            yield (k, s, pad, aligned, out_slice, res, gate, wino, w4, split, tiled, pw1x1)


def _dispatch_trace(stub, monkeypatch, case, rc):
    """(calls, records or the exception) of one ops.conv2d call, with and without ops.PROFILE."""
    from torch import nn

    from simplerecon_amd import ops
    k, s, pad, aligned, out_slice, res, gate, wino, w4, split, tiled, pw1x1 = case
    b, ci, co, h, w = 2, 8, 12, 8, 12
    stub.prefer_wino, stub.prefer_wino4, stub.rc = wino, w4, rc
    _lib.set_option("SR_WINO_SPLIT", split)
    monkeypatch.setattr(ops, "PW_TILED_MIN_ROWS", 1 if tiled else 100000)
    monkeypatch.setattr(ops, "USE_PW_1X1", pw1x1)
    trace = {}
    for profiled in (False, True):
        ops._SHAPE_QUERIES.clear()
        conv = nn.Conv2d(ci, co, k, stride=s, padding=k // 2, padding_mode="zeros" if pad == "tf_same" else pad)
        bn = nn.BatchNorm2d(co).eval()
        x = torch.zeros(b, h, w, ci + 3)[..., 1:1 + ci].permute(0, 3, 1, 2) if not aligned else \
            torch.zeros(b, ci, h, w).contiguous(memory_format=torch.channels_last)
        ho, wo = -(-h // s), -(-w // s)
        out = torch.zeros(b, ho, wo, co + 8)[..., 4:4 + co].permute(0, 3, 1, 2) if out_slice else None
        kw = dict(residual=torch.zeros(b, co, ho, wo).contiguous(memory_format=torch.channels_last), act="silu") if res \
            else dict(leaky=0.1)
        if gate:
            kw["gate"] = torch.ones(b, ci)
        prof = [] if profiled else None
        monkeypatch.setattr(ops, "PROFILE", prof)
        del stub[:], stub.args[:]
        try:
            with torch.no_grad():
                ops.conv2d(x, conv, out=out, bn=bn, tf_same=pad == "tf_same", **kw)
            if profiled:
                trace["records"] = [[n, f, list(shape), ex] for n, f, _, _, shape, ex in prof]
        except (ValueError, _lib.HipLibraryError) as e:
            trace["raises"] = f"{type(e).__name__}: {e}"
        # (profiled: without the query behind a record's name and executed FLOPs -- the records pin what it answered)
        trace["calls_profiled" if profiled else "calls"] = [
            _pinned_call(n, a) for n, a in stub.args if not (profiled and n == "sr_last_launch")]
    return trace


def _pinned_call(name, args):
    """[entry point, every non-pointer argument, "p" / None for each pointer]"""
    return [name] + [("p" if v is not None else None) if t is ctypes.c_void_p else
                     round(v.value if isinstance(v, ctypes.c_float) else v, 6) for v, t in zip(args, _lib.SIGNATURES[name][1])]


def _dispatch_traces(stub, monkeypatch):
    from simplerecon_amd import ops
    monkeypatch.setattr(ops, "_PACKED", weakref.WeakKeyDictionary())
    traces = {}
    saved = _lib.get_option("SR_WINO_SPLIT")
    try:
        for case in _dispatch_cases():
            cid = "-".join(map(str, case))
            rc = {}
            for step in range(6):
                t = _dispatch_trace(stub, monkeypatch, case, dict(rc))
                traces[f"{cid}/rc2x{step}"] = t
                launched = [c[0] for c in t["calls"] if c[0].endswith("_fwd")]
                if step == 0 and launched:
                    traces[f"{cid}/rc1"] = _dispatch_trace(stub, monkeypatch, case, {launched[0]: 1})
                if "raises" in t or not launched or launched[-1] in rc:
                    break
                rc[launched[-1]] = 2   # the entry point that served the call now answers SR_ERR_UNSUPPORTED
    finally:
        _lib.set_option("SR_WINO_SPLIT", saved)
    return json.loads(json.dumps(traces))


def test_conv2d_dispatch_matches_the_golden(stub, monkeypatch):
    """ops.conv2d calls the same entry points, falls back in the same order and writes the same PROFILE records (algorithmic
    FLOPs and shape; the name and the executed FLOPs are the launcher's to report -- here the stub's "stub:<entry point>" and
    None, on a GPU what tests/test_gpu_launch_records.py pins) as recorded in tests/golden/conv2d_dispatch.json.gz."""
    got = _dispatch_traces(stub, monkeypatch)
    with gzip.open(_GOLDEN_DISPATCH, "rt") as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    for cid in want:
        assert got[cid] == want[cid], cid


# ---- the conv training layer's launch trace, pinned -----------------------------------------------------------------------
# What autograd_ops._ConvBiasAct launches, forward and backward, over a grid of precisions (autocast dtype and the four 16-bit
# switches), library answers, layer shapes, operands, needed gradients and FUSED_ACT_BIAS: every call to an entry point that
# launches (pack calls included; pure queries are not part of it), in order, with the dtypes of the output and of what autograd
# saved and the dtype, shape and strides of every returned gradient.  Recorded in tests/golden/conv_layer_trace.json.gz by
# scripts/record_conv_layer_trace.py; a case that raises pins its exception.
_GOLDEN_LAYER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_layer_trace.json.gz")
_QUERIES = ("_supported", "_prefers", "_prefers_wino", "_bytes", "_floats")
# amp: the autocast dtype (None: no autocast region); store / io / mfma / wgrad: STORE_HALF, HALF_IO, MFMA16, MFMA16_WGRAD;
# p16: sr_conv16_prefers answers 0, 1, or "fwd" = 1 for the layer's own shape only (not for its transposed data gradient);
# p16w / wino: sr_conv16_wgrad_prefers / sr_conv_prefers_wino; x16: x (and the residual) arrive in the autocast dtype, as from
# a 16-bit layer before; sliced: x is a channel slice whose 16-bit rows are not 16-byte aligned; g32: the backward is handed a
# dense fp32 gradient (directly: the engine would cast it to the output's dtype); need: the inputs that require a gradient
# (x, weight, bias, residual); then: switches set between the forward and the backward.
_LAYER_CASE = dict(amp=None, store=False, io=False, mfma=0, wgrad=0, p16=1, p16w=1, wino=False, k=3, s=1, pads=None, b=2, ci=8,
                   co=16, bias=True, res=False, slope=0.1, x16=False, sliced=False, g32=False, need="xwbr", fused=True, then=None)
_LAYER_SWITCHES = dict(store="STORE_HALF", io="HALF_IO", mfma="MFMA16", wgrad="MFMA16_WGRAD", fused="FUSED_ACT_BIAS")


def _layer_cases():
    bf16, fp16 = "bfloat16", "float16"
    full = [dict()] + [dict(amp=bf16, io=io, mfma=m, wgrad=g) for io, m, g in
                       ((False, 0, 0), (True, 0, 0), (True, 1, 0), (True, 2, 0), (True, 1, 1), (True, 1, 2), (True, 2, 1), (True, 2, 2))] + \
        [dict(amp=fp16, io=io, mfma=m, wgrad=g) for io, m, g in ((False, 0, 0), (True, 0, 0), (True, 2, 0), (True, 2, 2))]
    few = [full[0], full[1], full[2], full[4], full[5], full[8], full[12]]
    shapes = [dict(k=1), dict(k=3), dict(k=3, wino=True), dict(k=1, s=2), dict(k=3, s=2), dict(k=3, pads=(1, 0, 1, 2)), dict(k=3, s=2, pads=(0, 0, 1, 1))]
    for prec in full:       # precision x shape x STORE_HALF (16 x 16 maps: 4096 elements, what _stash narrows) x arriving dtype
        for shape in shapes:
            for store in (False, True):
                for x16 in ((False, True) if prec.get("io") else (False,)):
                    yield dict(prec, **shape, store=store, x16=x16)
    variants = [dict(p16=0), dict(p16="fwd"), dict(p16w=0), dict(wino=True, res=True, bias=False),
                dict(co=6), dict(co=6, fused=False), dict(b=0), dict(b=0, need="w"),
                dict(bias=False), dict(res=True), dict(slope=None), dict(bias=False, res=True, slope=None), dict(bias=False, slope=None),
                dict(sliced=True), dict(sliced=True, res=True), dict(g32=True), dict(g32=True, slope=None, bias=False),
                dict(need="x"), dict(need="w"), dict(need="xwr", res=True), dict(need="wb"), dict(need="r", res=True),
                dict(fused=False), dict(fused=False, slope=None), dict(fused=False, bias=False),
                dict(then=dict(mfma=0)), dict(then=dict(wgrad=0)), dict(then=dict(mfma=2, wgrad=2)), dict(then=dict(fused=False))]
    for prec in few:        # every other axis, one or two at a time, where it can change a branch
        for shape in (shapes[0], shapes[1], shapes[4], shapes[5]):
            for var in variants:
                for x16 in ((False, True) if prec.get("io") else (False,)):
                    if var.get("sliced") and not x16 and prec.get("io"):   # (an fp32 slice is repacked by the cast: aligned)
                        continue
                    yield dict(prec, **shape, **var, store=bool(prec.get("mfma")), x16=x16)


def _layer_trace(stub, monkeypatch, case):
    from simplerecon_amd import autograd_ops
    c = dict(_LAYER_CASE, **case)
    amp = getattr(torch, c["amp"]) if c["amp"] else None
    monkeypatch.setattr(torch, "is_autocast_enabled", lambda *a: amp is not None)
    monkeypatch.setattr(torch, "get_autocast_dtype", lambda *a: amp or torch.float16)
    for key, name in _LAYER_SWITCHES.items():
        monkeypatch.setattr(autograd_ops, name, c[key])
    k, s, b, ci, co, h, w = c["k"], c["s"], c["b"], c["ci"], c["co"], 16, 16
    layer = (b, h, w, ci, co, k, s)
    stub.prefer16, stub.prefer16_wgrad, stub.prefer_wino = {layer} if c["p16"] == "fwd" else c["p16"], c["p16w"], c["wino"]
    pt, pl, pb, pr = c["pads"] or (k // 2,) * 4
    ho, wo = (h + pt + pb - k) // s + 1, (w + pl + pr - k) // s + 1
    dt = amp if c["x16"] else torch.float32
    x = torch.zeros(b, h, w, ci + 3, dtype=dt)[..., 1:1 + ci].permute(0, 3, 1, 2) if c["sliced"] else \
        torch.zeros(b, ci, h, w, dtype=dt).contiguous(memory_format=torch.channels_last)
    ins = dict(x=x.detach(), w=torch.zeros(co, ci, k, k), b=torch.zeros(co) if c["bias"] else None,
               r=torch.zeros(b, co, ho, wo, dtype=dt).contiguous(memory_format=torch.channels_last) if c["res"] else None)
    for name, t in ins.items():
        if t is not None:
            t.requires_grad_(name in c["need"])
    trace = {}
    pinned = lambda: [_pinned_call(n, a) for n, a in stub.args if not n.endswith(_QUERIES)]
    describe = lambda t: None if t is None else [str(t.dtype), list(t.shape), list(t.stride())]
    del stub[:], stub.args[:]
    try:
        out = autograd_ops._ConvBiasAct.apply(ins["x"], ins["w"], ins["b"], ins["r"], s, c["slope"], c["pads"])
        trace["forward"] = pinned()
        trace["out"] = describe(out)
        trace["saved"] = [None if t is None else str(t.dtype) for t in out.grad_fn.saved_tensors]
        for key, value in (c["then"] or {}).items():
            monkeypatch.setattr(autograd_ops, _LAYER_SWITCHES[key], value)
        del stub[:], stub.args[:]
        if c["g32"]:
            g = torch.zeros(out.shape).contiguous(memory_format=torch.channels_last)
            grads = dict(zip("xwbr", autograd_ops._ConvBiasAct.backward(out.grad_fn, g)))
        else:
            wanted = [n for n, t in ins.items() if t is not None and t.requires_grad]
            grads = dict(zip(wanted, torch.autograd.grad(out.sum(), [ins[n] for n in wanted], allow_unused=True)))
        trace["backward"] = pinned()
        trace["grads"] = {n: describe(grads.get(n)) for n in "xwbr"}
    except (ValueError, TypeError, RuntimeError, _lib.HipLibraryError) as e:
        trace["raises"] = f"{type(e).__name__}: {e}"
    return trace


def _layer_traces(stub, monkeypatch):
    from simplerecon_amd import autograd_ops

    def nhwc_any(t, name):   # autograd_ops._nhwc_any without its CUDA-device check
        return t if autograd_ops._is_nhwc_view(t) else t.contiguous(memory_format=torch.channels_last)
    monkeypatch.setattr(autograd_ops, "_nhwc_any", nhwc_any)
    # (the layer's wrappers leave an autocast-off region: that writes back the patched state it read on the way in)
    real = torch.is_autocast_enabled("cuda"), torch.get_autocast_dtype("cuda")
    traces = {}
    try:
        for case in _layer_cases():
            cid = ",".join(f"{k}={v}" for k, v in case.items() if v != _LAYER_CASE[k]) or "default"
            assert cid not in traces, cid
            traces[cid] = _layer_trace(stub, monkeypatch, case)
    finally:
        torch.set_autocast_enabled("cuda", real[0])
        torch.set_autocast_dtype("cuda", real[1])
    return json.loads(json.dumps(traces))


def test_conv_layer_launch_trace_matches_the_golden(stub, monkeypatch):
    """_ConvBiasAct launches the same kernels with the same arguments, saves the same dtypes and returns gradients of the same
    dtype, shape and strides as recorded in tests/golden/conv_layer_trace.json.gz."""
    got = _layer_traces(stub, monkeypatch)
    with gzip.open(_GOLDEN_LAYER, "rt") as f:
        want = json.load(f)
    assert sorted(got) == sorted(want)
    for cid in want:
        assert got[cid] == want[cid], cid
