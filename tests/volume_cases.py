"""Case tables of the plane-sweep path tests (tests/test_gpu_mlp_volume_bwd_paths.py, tests/test_gpu_dot_volume_channels.py)
with the launch rules of the kernels restated, so that tests/test_volume_cases_host.py can prove without a GPU that every
case reaches the code path it is listed for.

Restated from csrc/sr_mlp_volume_bwd.hip (sr_mlp_volume_bwd):
  total_items = B * ceil(h w / 32) work items, min(total_items, CUs) persistent workgroups; a workgroup takes a second
  item only when total_items > CUs (256 on an MI355X);  nt1 = ceil(Cin / 32) dW1 column tiles with Cin = 26 K + 20 for
  16-channel features, served by the instantiations NT1 = 4 / 7 / 10 / 13.
Restated from csrc/sr_dot_volume.hip (sr_pick_plane_split, sr_dot_volume_sweep) for the generic kernel (C != 16):
  S doubles while S < 16, tiles * S < 4096 and 2 S <= D (tiles = B * ceil(h w / 64));  S == 1: one wave per tile walks all
  planes ("nosplit");  S > 1 and tiles < 1024: single-wave workgroups along grid z + a separate argmax launch ("spread");
  otherwise S waves of one workgroup merge their argmax in LDS ("workgroup").

LeakyReLU kinks: at the persistent sizes (25 000 (pixel, plane) evaluations of 256 hidden units) some pre-activation lands
within fp32 rounding of zero and its derivative flips between 1 and 0.01 -- the fp32 and fp64 oracles then differ by up to
8e-2.  `at_size_reference` zeroes the cotangent at every (pixel, plane) where any float64 pre-activation of either hidden
layer is within KINK_BAND * max|z| of zero for that layer (the treatment of tests/bwd_cases.py for the conv kinks)."""
import functools

import numpy as np
import torch

import golden_cases as gc
import oracle
from parity import rel_err
from simplerecon_amd import synthetic
from simplerecon_amd.cost_volume import CostVolumeManager, FeatureVolumeManager

MI355X_CUS = 256
GRAD_KEYS = ("d_cur_feats", "d_src_feats", "dW1", "db1", "dW2", "db2", "dW3", "db3")
KINK_BAND = 1e-5           # of max|z| of the layer
KINK_SHARE_MAX = 0.03      # of the (pixel, plane) pairs
ORACLE_AGREE_MAX = 3e-5    # f32 oracle vs f64 oracle on every gradient (range-relative); the GPU bar is parity.TOL = 1e-4
SLOPE = 0.01               # nn.LeakyReLU default (reference networks.py:139)


# ------------------------------------------------------------------------------------------------ launch rules ----
def mlp_bwd_items(B, h, w):
    return B * ((h * w + 31) // 32)


def mlp_cin(K, C=16):
    return C * (K + 1) + 10 * K + 4


def mlp_bwd_nt1(K):
    nt1 = (mlp_cin(K) + 31) // 32
    return 4 if nt1 <= 4 else 7 if nt1 <= 7 else 10 if nt1 <= 10 else 13


def dot_plane_split(B, N, D):
    tiles, S = B * ((N + 63) // 64), 1
    while S < 16 and tiles * S < 256 * 16 and S * 2 <= D:
        S *= 2
    return S


def dot_launch_shape(B, h, w, D):
    """'nosplit' / 'spread' / 'workgroup' and the plane split S of the generic dot kernel."""
    S = dot_plane_split(B, h * w, D)
    if S == 1:
        return "nosplit", S
    return ("spread" if B * ((h * w + 63) // 64) < 4 * 256 else "workgroup"), S


# ------------------------------------------------------------------------------------------------ MLP backward ----
# persistent loop: more work items than CUs, so workgroups take a second item with live dW1 / dW2 accumulators; the last
# 32-pixel tile of an image is ragged in both (6391 = 199 * 32 + 23, 12319 = 384 * 32 + 31)
PERSISTENT_CASES = [
    dict(name="k2_b2_77x83", B=2, K=2, D=2, h=77, w=83, seed=3, mlp_seed=5),       # 400 items, NT1 = 4
    dict(name="k7_b1_97x127", B=1, K=7, D=2, h=97, w=127, seed=11, mlp_seed=7),    # 385 items, NT1 = 7, Cin = 202
]
# view counts: K = 1 (one (pixel, view) pass, 7 of 8 thread groups idle in the assembly), 4 (Cin = 124: last tile of NT1 = 4
# nearly full), 5 (Cin = 150: NT1 = 7 with two wholly unused column tiles), 9 and 11 (NT1 = 10; 11 fills it: Cin = 306),
# 12 (first of NT1 = 13)
VIEW_CASES = [dict(name=f"k{K}", B=1, K=K, D=2, h=10, w=21, seed=30 + K, mlp_seed=40 + K) for K in (1, 4, 5, 9, 11, 12)]
EDGE_CASE = dict(name="edge_k4", B=1, K=4, D=3, h=13, w=17, seed=7, mlp_seed=8, edge=True)
PIXEL_PLANES_CASE = dict(name="pixel_planes", B=2, K=2, D=3, h=11, w=19, seed=8, mlp_seed=9, pixel_planes=True)
LAYOUT_CASE = dict(name="layouts", B=2, K=3, D=3, h=13, w=17, seed=9, mlp_seed=10)
BATCH_CASE = dict(name="batch3", B=3, K=2, D=2, h=9, w=15, seed=12, mlp_seed=13)
FROZEN_CASE = dict(name="frozen_mlp", B=1, K=2, D=2, h=10, w=12, seed=14, mlp_seed=15)
SMALL_CASES = VIEW_CASES + [EDGE_CASE, PIXEL_PLANES_CASE, LAYOUT_CASE, BATCH_CASE, FROZEN_CASE]
MLP_CASES = PERSISTENT_CASES + SMALL_CASES

# ------------------------------------------------------------------------------------------- dot-product sweep ----
DOT_CHANNELS = (4, 8, 12, 24, 32)
DOT_SHAPES = {
    "nosplit": dict(B=1, K=2, D=1, h=13, w=17, seed=21),
    "spread": dict(B=2, K=3, D=5, h=37, w=29, seed=3),         # S = 4 over 5 planes: the last plane group is empty
    "workgroup": dict(B=4, K=2, D=5, h=120, w=137, seed=22),   # 1028 tiles, S = 4: the fourth wave has no plane
}
DOT_WORKGROUP_CHANNELS = (12, 32)
DOT_BWD_CASE = DOT_SHAPES["spread"]                            # the ragged 37x29 shape
DOT_BWD_EDGE_CASE = dict(B=1, K=4, D=4, h=20, w=28, seed=5, edge=True)
DOT_BWD_EDGE_CHANNELS = (12, 24)                               # the two scatter forms with idle lanes (64 % C != 0)
WARP_CASE = dict(B=2, K=3, C=8, D=3, h=19, w=23, seed=23)


# ------------------------------------------------------------------------------------------------ inputs ----------
def inputs(case):
    """CPU keyword arguments of the manager's forward with `depth_planes_bdhw` always given (computed on the CPU: the
    device and the oracle then sweep bit-identical planes)."""
    case = dict(case, C=case.get("C", 16))
    inp = gc.volume_inputs(case)
    if "depth_planes_bdhw" not in inp:
        mgr = CostVolumeManager(case["h"], case["w"], num_depth_bins=case["D"])
        inp["depth_planes_bdhw"] = mgr.generate_depth_planes(case["B"], inp["min_depth"], inp["max_depth"])
    return inp


def planes_np(case, inp):
    p = inp["depth_planes_bdhw"].numpy()
    return np.ascontiguousarray(p if case.get("pixel_planes") else p[:, :, 0, 0])


def manager(case):
    """The metadata-MLP manager of a case on the CPU (seeded weights)."""
    mgr = FeatureVolumeManager(case["h"], case["w"], num_depth_bins=case["D"], matching_dim_size=16,
                               num_source_views=case["K"])
    synthetic.seeded_fill_(mgr.mlp, seed=case["mlp_seed"])
    return mgr


def mlp_dict(mgr):
    sd = {k: v.detach().cpu().numpy() for k, v in mgr.mlp.state_dict().items()}
    return dict(W1=sd["net.0.weight"], b1=sd["net.0.bias"], W2=sd["net.2.weight"], b2=sd["net.2.bias"],
                W3=sd["net.4.weight"], b3=sd["net.4.bias"])


def cotangent(case):
    """dL/d cost_volume ~ N(0.25, 1).  The mean is there for db3 = sum(cotangent), a single number: with a zero-mean
    cotangent it is what is left of 25 000 cancelling terms at the persistent sizes, and its error relative to itself
    (6.7e-5 between the fp32 and fp64 oracles, measured) is the conditioning of that sum, not of any kernel."""
    rng = np.random.default_rng(7100 + case["seed"])
    return rng.standard_normal((case["B"], case["D"], case["h"], case["w"]), dtype=np.float32) + np.float32(0.25)


def _geom_args(inp):
    n = {k: np.ascontiguousarray(v.numpy()) for k, v in inp.items()}
    return (n["cur_feats"], n["src_feats"], n["src_Ks"], n["src_extrinsics"], n["src_poses"], n["cur_invK"])


def oracle_backward(case, inp, mlp, cot, precision="f64"):
    return oracle.mlp_volume_backward(cot, *_geom_args(inp), planes_np(case, inp), mlp, precision=precision)


def oracle_forward(case, inp, mlp, precision="f64"):
    return oracle.mlp_volume(*_geom_args(inp), planes_np(case, inp), mlp, precision=precision)[0]


def oracle_agreement(case, inp, mlp, cot):
    """max over the eight gradients of rel_err(f32 oracle, f64 oracle), and the f64 gradients."""
    g32, g64 = oracle_backward(case, inp, mlp, cot, "f32"), oracle_backward(case, inp, mlp, cot, "f64")
    return max(rel_err(g32[k], g64[k]) for k in GRAD_KEYS), g64


# ------------------------------------------------------------------------------------------------ kinks -----------
def preactivations_f64(case, inp, mlp):
    """float64 pre-activations (z1, z2 [B,D,h,w,128]) and output [B,D,h,w] of the MLP on oracle.mlp_input's float64 input
    vectors -- the network restated in numpy (Linear, LeakyReLU(0.01), Linear, LeakyReLU(0.01), Linear)."""
    B, D, h, w = case["B"], case["D"], case["h"], case["w"]
    args, planes = _geom_args(inp), planes_np(case, inp)
    F = np.empty((B, D, h, w, mlp_cin(case["K"])), np.float64)
    for b in range(B):
        for j in range(D):
            for y in range(h):
                for x in range(w):
                    d = planes[b, j, y, x] if planes.ndim == 4 else planes[b, j]
                    F[b, j, y, x] = oracle.mlp_input(*args, float(d), b, y, x, precision="f64")
    W1, b1, W2, b2, W3, b3 = (np.asarray(mlp[k], np.float64) for k in ("W1", "b1", "W2", "b2", "W3", "b3"))
    z1 = F @ W1.T + b1
    z2 = np.where(z1 > 0, z1, z1 * SLOPE) @ W2.T + b2
    out = (np.where(z2 > 0, z2, z2 * SLOPE) @ W3.T + b3)[..., 0]
    return z1, z2, out


def kink_cotangent(case, inp, mlp, cot):
    """(cotangent zeroed on the ambiguous (pixel, plane) pairs, their share).  The restated forward is first checked
    against oracle.mlp_volume in float64 (1e-8: both are float64 evaluations of the same network)."""
    z1, z2, out = preactivations_f64(case, inp, mlp)
    e = rel_err(out, oracle_forward(case, inp, mlp, "f64"))
    assert e <= 1e-8, f"{case['name']}: restated MLP forward differs from the float64 oracle by {e:.2e}"
    amb = (np.abs(z1) <= KINK_BAND * np.abs(z1).max()).any(-1) | (np.abs(z2) <= KINK_BAND * np.abs(z2).max()).any(-1)
    return np.where(amb, np.float32(0), cot), float(amb.mean())


@functools.lru_cache(maxsize=None)
def at_size_reference(name):
    """Inputs, kink-zeroed cotangent and oracle results of a persistent case, computed once per process:
    dict(inp, mgr, mlp, cot, share, agree, ref = float64 gradients, fwd = float64 volume).  Treat as read-only."""
    case = next(c for c in PERSISTENT_CASES if c["name"] == name)
    inp, mgr = inputs(case), manager(case)
    mlp = mlp_dict(mgr)
    cot, share = kink_cotangent(case, inp, mlp, cotangent(case))
    agree, ref = oracle_agreement(case, inp, mlp, cot)
    return dict(inp=inp, mgr=mgr, mlp=mlp, cot=cot, share=share, agree=agree, ref=ref,
                fwd=oracle_forward(case, inp, mlp, "f64"))


# ------------------------------------------------------------------------- ATen references (warp_features) --------
def dot_inputs(shape, C):
    return inputs(dict(shape, C=C))


def to_device(inp, device):
    return {k: v.to(device) for k, v in inp.items()}


def as_f64(inp):
    return {k: (v.double() if torch.is_floating_point(v) else v) for k, v in inp.items()}
