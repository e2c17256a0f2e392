"""The cases of the frame-preparation tests, shared by tests/golden/make_frames_golden.py (which writes the expected
results with Pillow and torch's CPU kernels) and the tests that load them."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# name -> (B, h, w, C, H, W)
COLOR_CASES = {
    "wide": (1, 97, 131, 3, 48, 67),        # non-integer factor of about 2; narrower than the 128-column tile ("tiles" spans several)
    "ragged": (1, 37, 53, 3, 11, 17),       # factor over 3, ragged
    "up": (1, 30, 40, 3, 48, 64),           # upscale
    "skip_rows": (1, 60, 80, 3, 60, 40),    # vertical pass skipped
    "skip_cols": (1, 60, 80, 3, 30, 80),    # horizontal pass skipped
    "same": (1, 64, 64, 3, 64, 64),         # no resize
    "steep": (1, 250, 333, 3, 30, 40),      # factor of about 8.3: the rows of a tile do not fit LDS
    "pixel": (1, 5, 7, 3, 1, 1),            # a single output pixel
    "grey": (1, 37, 53, 1, 11, 17),
    "four": (1, 37, 53, 4, 11, 17),
    "batch": (9, 37, 53, 3, 11, 17),        # distinct images
    "tiles": (2, 70, 300, 3, 35, 150),      # more than one tile both ways (output wider than 128, taller than 16)
}
FLIP_CASES = ("wide", "ragged")
OTHER_FILTERS = ("bicubic", "lanczos", "box", "hamming")
FILTER_CASES = ("ragged", "up")

# name -> (h, w, H, W); H None = the native size
DEPTH_CASES = {"down": (48, 64, 19, 25), "up": (19, 25, 48, 64), "same": (48, 64, None, None)}
DEPTH_SPECIALS = (0, 1, 2, 9999, 10000, 10001, 32767, 32768, 65535)   # millimetres: both comparisons' boundaries

TUPLE = dict(image_height=96, image_width=128, depth_height=24, depth_width=32, high_res_image_height=120,
             high_res_image_width=160, include_high_res_color=True, include_full_res_depth=True,
             include_full_depth_K=True)


def color_input(name):
    """Seeded noise with a block of 0 next to a block of 255 and a one-pixel checkerboard of the two, so that the
    clamps and the rounding of both passes are hit (filters with negative lobes overshoot at those edges)."""
    B, h, w, C = COLOR_CASES[name][:4]
    rng = np.random.default_rng(sorted(COLOR_CASES).index(name) + 100)
    img = rng.integers(0, 256, (B, h, w, C), dtype=np.uint8)
    img[:, : h // 3, : w // 3] = 0
    img[:, : h // 3, w // 3: 2 * (w // 3)] = 255
    yy, xx = np.mgrid[0:h, 0:w]
    board = (((yy + xx) & 1) * 255).astype(np.uint8)
    img[:, h - h // 3:, : w // 2] = board[None, h - h // 3:, : w // 2, None]
    return img


def depth_input(name):
    h, w = DEPTH_CASES[name][:2]
    rng = np.random.default_rng(sorted(DEPTH_CASES).index(name) + 200)
    d = rng.integers(300, 12000, (2, h, w)).astype(np.uint16)
    flat = d.reshape(2, -1)
    where = rng.permutation(h * w)[: 6 * len(DEPTH_SPECIALS)]
    flat[:, where] = np.tile(np.array(DEPTH_SPECIALS, dtype=np.uint16), 6)
    return d


def load(kind):
    return dict(np.load(os.path.join(GOLDEN, f"frames_{kind}.npz"), allow_pickle=False))
