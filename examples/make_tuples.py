"""Tuple file of one scan from its camera poses: the four modes of the reference's data_scripts/generate_test_tuples.py
(simplerecon_amd.keyframes), for scans that come without precomputed lists (ARKit, COLMAP, Scanniverse captures).

    python examples/make_tuples.py --poses scan.npy --mode dense_offline --scan my_scan --out my_scan_dense_offline.txt
                                   [--num-images-in-tuple 8] [--device cuda]

--poses: an [N,4,4] .npy of camera-to-world poses, one per VALID frame, in time order.  --mode: default (online tuples at
keyframes: the evaluation lists), offline (keyframes, sources from both sides in time), dense (every frame, sources from
the past), dense_offline (every frame, both sides).  --device: run the per-frame walks of the last three on that GPU;
without it everything runs on the host.  One line per tuple, `scan id0 id1 ... id7`, the reference frame first, ids =
row numbers of the pose file.  A frame whose walk finds fewer sources gets a shorter line (the first frames of a scan in
the online modes; the reference's dataset crawl fills those with random earlier frames afterwards).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from simplerecon_amd import keyframes as kf  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--poses", required=True, help="[N,4,4] .npy, camera-to-world")
    ap.add_argument("--mode", choices=("default", "offline", "dense", "dense_offline"), default="default")
    ap.add_argument("--num-images-in-tuple", type=int, default=8)
    ap.add_argument("--scan", default="scan")
    ap.add_argument("--out", required=True)
    ap.add_argument("--device", default=None, help="e.g. cuda: run the walks on the GPU (not for --mode default)")
    args = ap.parse_args()

    poses = np.load(args.poses)
    if poses.ndim != 3 or poses.shape[1:] != (4, 4):
        sys.exit(f"{args.poses}: expected [N,4,4] poses, got {poses.shape}")
    n = args.num_images_in_tuple - 1
    if args.mode == "default":
        if args.device is not None:
            sys.exit("--mode default is one online buffer fed frame by frame: it runs on the host")
        samples = kf.default_dvmvs_tuples(args.scan, poses.astype(np.float64), [None] * len(poses), n)
    else:
        make = {"offline": kf.offline_dvmvs_tuples, "dense": kf.dense_dvmvs_tuples,
                "dense_offline": kf.offline_dense_dvmvs_tuples}[args.mode]
        samples = make(args.scan, poses, n, device=args.device)
    kf.write_tuple_file(args.out, samples)
    short = sum(len(s["indices"]) < args.num_images_in_tuple for s in samples)
    print(f"{args.out}: {len(samples)} tuples of {len(poses)} frames ({args.mode}), {short} with fewer than "
          f"{args.num_images_in_tuple} frames")


if __name__ == "__main__":
    main()
