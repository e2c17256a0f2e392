"""Writes tests/golden/jitter.npz: for the small colour-jitter cases (tests/jitter_cases.py GOLDEN_CASES) the resized
8-bit inputs, the parameters and the float64 result of tests/jitter_oracle.py rounded to fp32, un-normalised.

    python tests/golden/make_jitter_golden.py

The file pins the oracle: a change to it shows as a difference from what is stored.  It is not torchvision's output
(the package is absent here); parity against the package is unpinned."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import jitter_cases as jc  # noqa: E402


def main():
    out = {"torch_version": np.array(torch.__version__)}
    for name in jc.GOLDEN_CASES:
        _, _, p, flip, small = jc.case(name)
        out[f"in_{name}"] = small
        out[f"order_{name}"] = p.order
        out[f"factors_{name}"] = p.factors
        out[f"on_{name}"] = np.array(p.on)
        out[f"flip_{name}"] = np.array(flip)
        out[f"f32_{name}"] = jc.oracle(name, False, torch.float64).float().numpy()
    np.savez_compressed(jc.GOLDEN, **out)
    size = os.path.getsize(jc.GOLDEN)
    assert size < 256 * 1024, size
    print(jc.GOLDEN, size, "bytes")


if __name__ == "__main__":
    main()
