"""Writes tests/golden/pcfusion_<case>.npz: the reference's own process_scene (tools/torch_point_cloud_fusion.py) run
on the CPU for the cases of tests/pc_cases.py.  Needs a checkout of the reference; pass its root as the argument.
torch.Tensor.cuda is replaced by the identity in this process only, so the reference's .cuda() calls stay on the CPU.

    python tests/golden/make_pc_golden.py /path/to/simplerecon
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import pc_cases  # noqa: E402


def main(ref_root):
    sys.path.insert(0, ref_root)
    torch.Tensor.cuda = lambda self, *a, **k: self
    from tools import torch_point_cloud_fusion as tpf
    for name in pc_cases.CASES:
        sc, zt, nt = pc_cases.scene(name)
        with torch.no_grad():
            pts, rgb, valid = tpf.process_scene(sc["depths"], sc["images"], sc["cam_T_world"], sc["K"], zt, nt)
        path = os.path.join(HERE, f"pcfusion_{name}.npz")
        np.savez_compressed(path, fused_pts=pts.astype(np.float32), fused_rgb=rgb.astype(np.uint8),
                            all_valid=valid.astype(bool))
        print(f"{path}: {len(pts)} points of {valid.size} pixels")


if __name__ == "__main__":
    main(sys.argv[1])
