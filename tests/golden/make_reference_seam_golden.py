"""Generates tests/golden/reference_seam.npz: what tests/test_reference_seam.py needs to know about the UPSTREAM
reference's classes, recorded from the classes themselves on CPU.

Run in the build container only (needs /root/reference):

    python tests/golden/make_reference_seam_golden.py

Recorded, for the three cost-volume managers (the configurations of the seam test): the class name, the attributes
`cost_volume.to_hip` reads, the state-dict keys in order with shapes and dtypes, the values of every non-MLP buffer, the
MLP's layer widths, and `generate_depth_planes` on the test's inputs.  For CVEncoder, DepthDecoderPP, MLP and
ResnetMatchingEncoder: the state-dict keys in order with shapes and dtypes.  For utils/geometry_utils.pose_distance: its
outputs on the test's poses.  Everything structural goes into the JSON string `meta`, every array under its own name.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refshim  # noqa: E402
from simplerecon_amd import synthetic  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reference_seam.npz")
H, W, D = 12, 16, 8                                          # the shapes and cases of tests/test_reference_seam.py
MANAGER_CASES = [("dot", 3), ("mlp", 7), ("mlp", 2), ("fast", 5)]
ENC_CH, CV_OUT = [24, 48, 64, 160, 256], [64, 128, 256, 384]
ATTRS = ("matching_height", "matching_width", "num_depth_bins", "matching_dim_size", "num_source_views")


def _layout(module):
    return [[k, list(v.shape), str(v.dtype).replace("torch.", "")] for k, v in module.state_dict().items()]


def _manager(cv, kind, K):
    torch.manual_seed(3)
    if kind == "dot":
        return cv.CostVolumeManager(matching_height=H, matching_width=W, num_depth_bins=D)
    cls = cv.FeatureVolumeManager if kind == "mlp" else cv.FastFeatureVolumeManager
    return cls(matching_height=H, matching_width=W, num_depth_bins=D, mlp_channels=[202, 128, 128, 1],
               matching_dim_size=16, num_source_views=K)


def main():
    cv, nets, layers, geo, gen = refshim.import_reference()
    meta, arrays = {"managers": {}, "layouts": {}}, {}
    for kind, K in MANAGER_CASES:
        tag = f"{kind}{K}"
        m = _manager(cv, kind, K)
        rec = {"class": type(m).__name__, "attrs": {a: getattr(m, a) for a in ATTRS if hasattr(m, a)},
               "state_dict": _layout(m)}
        for k, v in m.state_dict().items():
            if not k.startswith("mlp."):
                arrays[f"{tag}/{k}"] = v.numpy()
        if hasattr(m, "mlp"):
            lin = [x for x in m.mlp.net if isinstance(x, torch.nn.Linear)]
            rec["mlp_channels"] = [lin[0].in_features] + [x.out_features for x in lin]
        inp = synthetic.cost_volume_inputs(2, K, 16, H, W, seed=1)
        arrays[f"{tag}/planes"] = m.generate_depth_planes(2, inp["min_depth"], inp["max_depth"]).numpy()
        meta["managers"][tag] = rec

    meta["layouts"]["CVEncoder"] = _layout(nets.CVEncoder(num_ch_cv=D, num_ch_enc=ENC_CH[1:], num_ch_outs=CV_OUT))
    meta["layouts"]["DepthDecoderPP"] = _layout(nets.DepthDecoderPP(ENC_CH[:1] + CV_OUT))
    meta["layouts"]["MLP"] = _layout(nets.MLP([202, 128, 128, 1], disable_final_activation=True))
    meta["layouts"]["ResnetMatchingEncoder"] = _layout(nets.ResnetMatchingEncoder(18, 16, pretrained=False).eval())

    poses, _ = synthetic.poses(3, 5, seed=2)
    for j, v in enumerate(geo.pose_distance(torch.from_numpy(poses.reshape(-1, 4, 4)))):
        arrays[f"pose_distance/{j}"] = v.numpy()

    np.savez_compressed(OUT, meta=np.array(json.dumps(meta, sort_keys=True)), **arrays)
    print(f"wrote {OUT}: {len(arrays)} arrays")


if __name__ == "__main__":
    main()
