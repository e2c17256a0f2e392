"""The stored scenes of the rasteriser tests (tests/golden/raster_*.npz, written by tests/golden/make_raster_golden.py)
and the cameras they are rendered with."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SCENES = ("grid", "room", "occluder", "near", "junk")
SIZES = ((72, 96), (67, 101))          # (H, W): the 96 x 72 image and an odd one
OFFSETS = (0.0, 0.5)
ZNEAR = 0.05


def load(name):
    with np.load(os.path.join(GOLDEN, f"raster_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


def intrinsics(H, W):
    """[4,4] fp32: focal length 0.9 W, principal point off the image centre by a fraction of a pixel."""
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = 0.9 * W
    K[0, 2] = (W - 1) / 2.0 + 0.3
    K[1, 2] = (H - 1) / 2.0 - 0.2
    return K


def configs():
    return [(s, H, W, o) for s in SCENES for (H, W) in SIZES for o in OFFSETS]
