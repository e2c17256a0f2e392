"""Times the colour jitter for one batch-8 set of tuples (8 tuples x 8 views = 64 frames), inputs resident on the
device: 64 colour images 968 x 1296 -> 384 x 512.  Device events around each repeat, warm-up first, median of the
repeats with the spread.

    python scripts/bench_jitter.py [--repeats 30] [--warmup 5] [--out profiles/jitter_prepare.json]

Three things are timed:
  prepare_color            the plain colour path (resize + to_tensor + normalise in one launch)
  prepare_color_jittered   resize to 8 bits, then the two jitter launches (mean pass, apply pass)
  torch_ops                the same jitter composed from torch operations on the device, frame by frame, from the rule
                           of tests/jitter_oracle.py, on the already resized images; the flip and normalisation included
and the two jitter launches alone (the resize taken out), against the 18 bytes per pixel they need: both passes read
the 3-byte pixel, the apply pass writes three floats.  There is no CPU path: without a GPU this script fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jitter_oracle  # noqa: E402
from simplerecon_amd import _lib, frames  # noqa: E402

N, CH, CW, H, W = 64, 968, 1296, 384, 512
STREAM_CEILING = 6.0e12      # bytes/s: the plain-stream ceiling of DESIGN.md 3.4


def gpu_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return {"ms_median": statistics.median(out), "ms_min": min(out), "ms_max": max(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jitter_prepare.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 repeats")
    dev = torch.device("cuda", 0)
    c = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (N, CH, CW, 3), dtype=np.uint8)).to(dev)
    params = frames.jitter_params(N, generator=torch.Generator().manual_seed(0))
    small = frames.resize_u8(c, H, W)
    table = torch.from_numpy(params.table()).to(dev)
    nbytes = int(_lib.lib().sr_frames_jitter_scratch_bytes(N, H, W))
    scratch = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    out = torch.empty((N, 3, H, W), dtype=torch.float32, device=dev)

    def launches():
        _lib.call("sr_frames_jitter", dev, small, N, H, W, table, out, 0, 1, scratch, nbytes)

    def torch_ops():
        return jitter_oracle.prepare(small, params.order, params.factors, params.on, flip=False, normalize=True)

    result = {"frames": N, "color_in": [CH, CW], "color_out": [H, W], "repeats": a.repeats, "warmup": a.warmup,
              "device": torch.cuda.get_device_name(0), "steps": {}}
    result["steps"]["prepare_color"] = gpu_ms(lambda: frames.prepare_color(c, H, W), a.warmup, a.repeats)
    result["steps"]["prepare_color_jittered"] = gpu_ms(lambda: frames.prepare_color_jittered(c, H, W, params), a.warmup,
                                                       a.repeats)
    result["steps"]["resize_u8"] = gpu_ms(lambda: frames.resize_u8(c, H, W), a.warmup, a.repeats)
    jl = result["steps"]["jitter_launches"] = gpu_ms(launches, a.warmup, a.repeats)
    needed = N * H * W * 18
    jl.update(needed_bytes=needed, bytes_per_pixel=18, bytes_per_s=needed / (jl["ms_median"] * 1e-3),
              share_of_stream_ceiling=needed / (jl["ms_median"] * 1e-3) / STREAM_CEILING)
    result["steps"]["torch_ops"] = gpu_ms(torch_ops, a.warmup, a.repeats)
    # the composition agrees with the kernels (its own device roundings: a few ulp), so the same work was timed
    launches()
    result["torch_ops_max_abs_difference"] = float((torch_ops() - out).abs().max())
    result["torch_ops_over_jitter_launches"] = result["steps"]["torch_ops"]["ms_median"] / jl["ms_median"]
    result["jittered_over_plain"] = result["steps"]["prepare_color_jittered"]["ms_median"] / \
        result["steps"]["prepare_color"]["ms_median"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
