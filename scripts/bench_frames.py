"""Times frame preparation for one batch-8 set of tuples (8 tuples x 8 views = 64 frames), inputs resident on the
device: 64 colour images 968 x 1296 -> 384 x 512, the same -> 480 x 640 (the high-res variant), and 64 depth maps
480 x 640 -> 192 x 256.  Device events around each repeat, warm-up first, median of the repeats.

    python scripts/bench_frames.py [--repeats 30] [--warmup 5] [--out profiles/frames_prepare.json]

Compulsory bytes of a step: its uint8 / uint16 input read once plus its outputs written once.  Where Pillow imports,
the same resizes and conversions run on 16 host threads for comparison (one frame per task); where it does not, the
comparison is recorded as not made.  There is no CPU path for the GPU side: without a GPU this script fails."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from simplerecon_amd import frames  # noqa: E402

N, CH, CW, DH, DW = 64, 968, 1296, 480, 640
STREAM_CEILING = 6.0e12      # bytes/s: the plain-stream ceiling of DESIGN.md 3.4
MODEL_STEP_MS = 25.5         # the model's batch-8 step (README headline)


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
    return statistics.median(out), min(out), max(out)


def pillow_ms(colors, depths, threads, repeats):
    try:
        from PIL import Image
    except ImportError:
        return None
    from concurrent.futures import ThreadPoolExecutor
    mean, std = (torch.tensor(v)[:, None, None] for v in (frames.IMAGENET_MEAN, frames.IMAGENET_STD))

    def one(i):
        img = Image.fromarray(colors[i], "RGB")
        for H, W in ((384, 512), (480, 640)):
            small = np.asarray(img.resize((W, H), resample=Image.BILINEAR))
            torch.from_numpy(small).permute(2, 0, 1).contiguous().float().div(255).sub_(mean).div_(std)
        d = np.asarray(Image.fromarray(depths[i]).resize((256, 192), resample=Image.NEAREST)).astype(np.int32)
        d = torch.from_numpy(d).float() * 1e-3
        ok = (d > 1e-3) & (d < 10.0)
        d[~ok] = float("nan")
    torch.set_num_threads(1)          # the parallelism is across frames, as in a DataLoader's workers
    times = []
    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(one, range(len(colors))))
        for _ in range(repeats):
            t0 = time.perf_counter()
            list(pool.map(one, range(len(colors))))
            times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frames_prepare.json"))
    a = ap.parse_args()
    if a.repeats < 20:
        ap.error("at least 20 repeats")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    colors = rng.integers(0, 256, (N, CH, CW, 3), dtype=np.uint8)
    depths = rng.integers(0, 12000, (N, DH, DW)).astype(np.uint16)
    c, d = torch.from_numpy(colors).to(dev), torch.from_numpy(depths).to(dev)
    steps = {
        "color_384x512": (lambda: frames.prepare_color(c, 384, 512), c.numel() + N * 3 * 384 * 512 * 4),
        "color_480x640": (lambda: frames.prepare_color(c, 480, 640), c.numel() + N * 3 * 480 * 640 * 4),
        "depth_192x256": (lambda: frames.prepare_depth(d, 192, 256), d.numel() * 2 + N * 192 * 256 * 9),
    }
    result = {"frames": N, "color_in": [CH, CW], "depth_in": [DH, DW], "repeats": a.repeats, "warmup": a.warmup,
              "device": torch.cuda.get_device_name(0), "steps": {}}
    for name, (fn, nbytes) in steps.items():
        med, lo, hi = gpu_ms(fn, a.warmup, a.repeats)
        result["steps"][name] = {"ms_median": med, "ms_min": lo, "ms_max": hi, "compulsory_bytes": nbytes,
                                 "bytes_per_s": nbytes / (med * 1e-3),
                                 "share_of_stream_ceiling": nbytes / (med * 1e-3) / STREAM_CEILING}

    def everything():
        for fn, _ in steps.values():
            fn()
    med, lo, hi = gpu_ms(everything, a.warmup, a.repeats)
    total = sum(b for _, b in steps.values())
    result["all"] = {"ms_median": med, "ms_min": lo, "ms_max": hi, "compulsory_bytes": total,
                     "bytes_per_s": total / (med * 1e-3), "share_of_stream_ceiling": total / (med * 1e-3) / STREAM_CEILING,
                     "model_step_ms": MODEL_STEP_MS, "share_of_model_step": med / MODEL_STEP_MS}
    result["paths"] = dict(frames.path_counts)
    cpu = pillow_ms(colors, depths, a.threads, 3)
    result["pillow"] = {"threads": a.threads, "ms_median": cpu, "repeats": 3} if cpu is not None else \
        {"comparison": "not made: Pillow does not import here"}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
