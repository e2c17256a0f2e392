"""The cases of the colour-jitter tests, shared by tests/golden/make_jitter_golden.py, tests/test_jitter_host.py and
tests/test_gpu_jitter.py, and the tolerance rule.  A case is (input images uint8 [B,h,w,3], output size, JitterParams,
flip); its oracle input is the Pillow-exact resize of tests/frames_oracle.py."""
import functools
import itertools
import os

import numpy as np
import torch

import frames_oracle
import jitter_oracle
from simplerecon_amd import frames

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jitter.npz")
ORDERS = list(itertools.permutations(range(4)))          # 24
DEFAULT = (0.2, 0.2, 0.2, 0.2)                           # the loader's ColorJitter(0.2, 0.2, 0.2, 0.2)
EDGE_FACTORS = ((0.8, 0.8, 0.8, -0.2), (1.2, 1.2, 1.2, 0.2), (0.0, 0.0, 0.0, 0.5), (2.0, 2.0, 2.0, -0.5))
CONTRAST_FIRST, CONTRAST_LAST = (1, 0, 2, 3), (0, 2, 3, 1)
CONTRAST_AFTER_HUE = (0, 3, 1, 2)


def cube_image():
    """64 x 64: the 16^3 lattice of channel values {0, 17, ..., 255} -- greys, primaries, black, white, every tie of
    the largest channel."""
    v = (np.arange(16) * 17).astype(np.uint8)
    r, g, b = np.meshgrid(v, v, v, indexing="ij")
    return np.stack([r, g, b], axis=-1).reshape(64, 64, 3)


def noise(seed, B, h, w):
    return np.random.default_rng(seed).integers(0, 256, (B, h, w, 3), dtype=np.uint8)


def default_draws(seed, n):
    """n draws from the default ranges, [n,4] float64 (fp32 values, as uniform_ gives them)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([0.8, 0.8, 0.8, -0.2]), np.array([1.2, 1.2, 1.2, 0.2])
    return (lo + (hi - lo) * rng.random((n, 4))).astype(np.float32).astype(np.float64)


def _params(order, factors, on=(True, True, True, True)):
    order = np.asarray(order).reshape(-1, 4)
    factors = np.asarray(factors, dtype=np.float64).reshape(-1, 4)
    return frames.JitterParams.from_values(order, *[factors[:, k] if on[k] else None for k in range(4)])


def _cube():
    return np.repeat(cube_image()[None], 24, axis=0), (64, 64), _params(ORDERS, default_draws(1, 24)), False


def _edges():
    order = [o for f in EDGE_FACTORS for o in (CONTRAST_FIRST, CONTRAST_LAST)]
    factors = [f for f in EDGE_FACTORS for _ in range(2)]
    return np.repeat(cube_image()[None], 8, axis=0), (64, 64), _params(order, factors), False


def _ragged():
    rng = np.random.default_rng(2)
    order = [ORDERS[i] for i in rng.permutation(24)[:3]]
    return noise(3, 3, 50, 71), (37, 53), _params(order, default_draws(4, 3)), True


def _several_groups():
    return noise(5, 1, 192, 256), (192, 256), _params([CONTRAST_AFTER_HUE], default_draws(6, 1)), False


def _strided():
    # more workgroups than SR_FRAMES_JITTER_MAX_PARTIALS (133 of 256 threads x 4 pixels): the mean pass strides
    return noise(7, 1, 272, 500), (272, 500), _params([CONTRAST_AFTER_HUE], default_draws(8, 1)), True


def _off(on):
    def make():
        order = [ORDERS[(5 * i + 3) % 24] for i in range(2)]
        return np.repeat(cube_image()[None], 2, axis=0), (64, 64), _params(order, default_draws(9, 2), on), False
    return make


OFF_SUBSETS = [on for on in itertools.product((False, True), repeat=4) if not all(on)]       # 15, "all off" included
CASES = {"cube": _cube, "edges": _edges, "ragged": _ragged, "several_groups": _several_groups, "strided": _strided}
CASES.update({"off_" + "".join("01"[v] for v in on): _off(on) for on in OFF_SUBSETS})
GOLDEN_CASES = ("ragged", "edges2", "off1")               # small ones: the file stays under 256 KB


def _part(name, lo, hi):
    def make():
        img, size, p, flip = CASES[name]()
        return img[lo:hi], size, frames.JitterParams(p.order[lo:hi], p.factors[lo:hi], p.on), flip
    return make


CASES["edges2"] = _part("edges", 6, 8)       # factors 2 with hue -0.5, contrast first and last
CASES["off1"] = _part("off_1011", 0, 1)      # contrast off


@functools.lru_cache(maxsize=None)
def case(name):
    """(images, (H, W), params, flip, resized uint8 [B,H,W,3])."""
    img, (H, W), params, flip = CASES[name]()
    return img, (H, W), params, flip, frames_oracle.resize_u8(img, H, W)


@functools.lru_cache(maxsize=None)
def oracle(name, normalize=False, dtype=torch.float64):
    """The oracle of a case, computed once per (case, normalize, dtype) and shared: treat it as read-only."""
    _, _, p, flip, small = case(name)
    return jitter_oracle.prepare(small, p.order, p.factors, p.on, flip=flip, normalize=normalize, dtype=dtype)


def e32(name):
    """max |oracle_fp32 - oracle_fp64| of the case's un-normalised result: what fp32 roundings alone amount to."""
    return float((oracle(name, False, torch.float32).double() - oracle(name, False, torch.float64)).abs().max())


def bound(name, normalize=False):
    """The tolerance against the float64 oracle: max(4 e32, 2^-22) un-normalised; divided by 0.224 plus 2^-21 after
    the normalisation.  Factor 4: the kernel may differ from torch's roundings by the order of the mean's sum, by its
    division sequence and by contraction, each a rounding of the size e32 is made of; hue passes an upstream
    difference on multiplied by at most 6, which e32 already contains."""
    b = max(4.0 * e32(name), 2.0 ** -22)
    return b / 0.224 + 2.0 ** -21 if normalize else b


def load_golden():
    return dict(np.load(GOLDEN, allow_pickle=False))
