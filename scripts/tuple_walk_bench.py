"""Times the dense tuple modes (simplerecon_amd.keyframes) on a 2 000-frame scan, device path against host path in one run.

    python scripts/tuple_walk_bench.py [--frames 2000] [--repeats 20] [--out profiles/tuple_walk.txt]

Two streams from tests/tuple_cases.figure_eight: the recipe of the golden stream (a) stretched to --frames frames (the camera
rests for a tenth of the scan), and one in which it rests for half of it, which makes the walks long.  Per stream and mode:
  host      the host path, wall clock, once, on every --host-stride-th frame and scaled by the stride: the walks are
            independent and the whole scan takes minutes (stride 1 times all of it)
  device    the public function with device="cuda", wall clock around it ending in a synchronise: pose checks, the
            host-to-device copy, both launches, the copy back and the Python lists
  gpu part  device events around [copy of the poses to the device, inverse + walk launches, copy of the indices back]
  kernels   device events around the two launches with the poses resident; the walk launch alone
Device numbers are medians over --repeats runs after a warm-up, with the range.  The tuples of the two paths are compared
(reference frame, set of sources) at the frames the host path ran.  Needs a GPU: there is no fallback."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import tuple_cases as tc  # noqa: E402
from simplerecon_amd import _lib  # noqa: E402
from simplerecon_amd import keyframes as kf  # noqa: E402

MODES = {"dense_offline": (kf.offline_dense_dvmvs_tuples, lambda p, n, i: kf.compute_offline_tuple(p, n, i, p[i]), True, 60),
         "dense": (kf.dense_dvmvs_tuples, kf._dense_tuple, False, 30)}


def events_ms(fn, repeats):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return times


def wall_ms(fn, repeats):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return times


def fmt(times):
    return f"{statistics.median(times):9.3f} ms  (min {min(times):.3f}, max {max(times):.3f}, n={len(times)})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=2000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--host-stride", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tuple_walk.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("no GPU: this script measures the device path")
    dev = torch.device("cuda")
    N, n = args.frames, 7
    lines = [f"# python scripts/tuple_walk_bench.py --frames {N} --repeats {args.repeats} --host-stride {args.host_stride}",
             f"# {torch.cuda.get_device_name(0)}, {_lib.lib().sr_target_arch().decode()}, torch {torch.__version__}; "
             f"{N} frames, {n} sources per tuple, fp64",
             "# host = this package's host path (numpy, one process), timed on every "
             f"{args.host_stride}th frame and multiplied by {N / len(range(0, N, args.host_stride)):g}; device = the same "
             "functions with device='cuda', all frames"]
    streams = {"rest 10 % (stream (a) stretched)": tc.figure_eight(N, 1),
               "rest 50 %": tc.figure_eight(N, 1, rest=(0.25, 0.75))}
    refs = torch.arange(N, dtype=torch.int32, device=dev)
    for title, poses in streams.items():
        lines.append(f"\n== {title} ==")
        for mode, (fn, one_frame, both, size) in MODES.items():
            frames = range(0, N, args.host_stride)
            t = time.perf_counter()
            host = [one_frame(poses, n, i) for i in frames]
            host_s = (time.perf_counter() - t) * N / len(frames)
            device = {s["indices"][0]: s for s in fn("scan", poses, n, device=dev)}
            host = [s for s in host if s["indices"][0] in device or len(s["indices"]) > 1]   # (frame 0 has no tuple)
            same = tc.tuples_as_comparable([device[s["indices"][0]] for s in host]) == tc.tuples_as_comparable(host)
            resident = torch.from_numpy(poses).to(dev)
            inverses = kf.pose_inverse(resident)
            indices = torch.empty((N, 1 + n), dtype=torch.int32, device=dev)
            counts = torch.empty((N,), dtype=torch.int32, device=dev)

            def gpu_part():
                idx, _ = kf.walk_tuples(torch.from_numpy(poses).to(dev), refs, n, both, size)
                return idx.cpu()

            def walk_only():
                _lib.call("sr_tuple_walk_f64", dev, resident, inverses, N, refs, N, int(both), size, size, 0.1, 0.15, 0.0, n,
                          indices, counts)

            e2e = wall_ms(lambda: fn("scan", poses, n, device=dev), args.repeats)
            part = events_ms(gpu_part, args.repeats)
            kernels = events_ms(lambda: kf.walk_tuples(resident, refs, n, both, size), args.repeats)
            walk = events_ms(walk_only, args.repeats)
            med = statistics.median(e2e)
            lines += [f"{mode}: {len(device)} tuples, device tuples == host tuples at {len(host)} frames: {same}",
                      f"  host                     {host_s * 1e3:9.1f} ms  (once, scaled)",
                      f"  device, public function  {fmt(e2e)}   host / device = {host_s * 1e3 / med:.0f} x",
                      f"  gpu part (copy, 2 launches, copy back) {fmt(part)}",
                      f"  kernels (inverse + walk) {fmt(kernels)}",
                      f"  walk kernel alone        {fmt(walk)}"]
            print("\n".join(lines[-6:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
