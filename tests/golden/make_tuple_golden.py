"""Records tests/golden/tuple_modes.npz: what the UPSTREAM reference's offline / dense / dense_offline tuple generators
(data_scripts/generate_test_tuples.py) and its SimpleBuffer / OfflineKeyframeBuffer (tools/keyframe_buffer.py) give on the
streams of tests/tuple_cases.py.  CPU only, where the reference tree exists:

    python tests/golden/make_tuple_golden.py

The reference's own functions run unmodified; they are wrapped at record time to count what the streams are there to
provoke (buffer overflow, rejections by an entry that is not the newest) and to measure how far every decision is from its
threshold.  The file is refused unless the events occur and every admission distance is 1e-9 clear of the keyframe
distance and every source choice 1e-9 clear of the next penalty: conditions on the INPUTS, under which an fp64
implementation with another inverse or summation order (rounding of order 1e-15) takes the same decisions."""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refshim  # noqa: E402
import tuple_cases as tc  # noqa: E402

MARGIN = 1e-9


def import_generator():
    """data_scripts/generate_test_tuples.py; its `options` / `utils.dataset_utils` imports (the crawl's, unused by the four
    tuple functions) get empty stand-ins when they do not import here."""
    kb = refshim.import_keyframe_buffer()
    for name, attrs in (("options", {}), ("utils.dataset_utils", {"get_dataset": None})):
        try:
            importlib.import_module(name)
        except Exception:
            if "." in name and name.split(".")[0] not in sys.modules:
                sys.modules[name.split(".")[0]] = types.ModuleType(name.split(".")[0])
            mod = types.ModuleType(name)
            mod.__dict__.update(attrs)
            sys.modules[name] = mod
    gen = importlib.import_module("data_scripts.generate_test_tuples")
    assert gen.tools.keyframe_buffer is kb
    return kb, gen


class Probe:
    """Wraps the reference's pose_distance, OfflineKeyframeBuffer.try_new_keyframe and
    get_best_measurement_frames_for_0index for the time of one recording."""

    def __init__(self, kb):
        self.kb = kb
        self.reset()

    def reset(self):
        self.overflows = self.nonlast_rejections = self.walks_overflowed = 0
        self.admission_margin = self.penalty_margin = np.inf
        self.ranked = []
        self._calls = 0
        self._scoring = False
        self._walk_overflowed = False

    def __enter__(self):
        kb, probe = self.kb, self
        self._saved = (kb.pose_distance, kb.OfflineKeyframeBuffer.try_new_keyframe,
                       kb.OfflineKeyframeBuffer.get_best_measurement_frames_for_0index)
        pose_distance, try_new, best = self._saved

        def counted_pose_distance(a, b):
            out = pose_distance(a, b)
            if not probe._scoring:
                probe._calls += 1
                probe.admission_margin = min(probe.admission_margin, abs(out[0] - kb.DVMVS_Config.test_keyframe_pose_distance))
            return out

        def counted_try_new(buf, pose, image, index=None):
            before, probe._calls = len(buf.buffer), 0
            code = try_new(buf, pose, image, index=index)
            if code == 1 and before == buf.buffer.maxlen:
                probe.overflows += 1
                probe._walk_overflowed = True
            if code == 2 and probe._calls < before:      # the loop broke before it reached the newest entry
                probe.nonlast_rejections += 1
            return code

        def counted_best(buf, n):
            probe._scoring = True
            try:
                frames = list(buf.buffer)[1:]
                row = []
                if frames:
                    pens = []
                    for f in frames:
                        _, r_m, t_m = pose_distance(frames[0][0], f[0])
                        pens.append(float(buf.calculate_penalty(t_m, r_m)))
                    take = min(n, len(frames) - 1)
                    order = sorted(range(len(frames)), key=lambda i: (pens[i], i))
                    if take >= 1:
                        probe.penalty_margin = min(probe.penalty_margin, pens[order[take]] - pens[order[take - 1]])
                    row = [frames[i][2] for i in order[:take]]
                probe.ranked.append(row)
                probe.walks_overflowed += probe._walk_overflowed
                probe._walk_overflowed = False
                return best(buf, n)
            finally:
                probe._scoring = False

        kb.pose_distance = counted_pose_distance
        kb.OfflineKeyframeBuffer.try_new_keyframe = counted_try_new
        kb.OfflineKeyframeBuffer.get_best_measurement_frames_for_0index = counted_best
        return self

    def __exit__(self, *exc):
        kb = self.kb
        (kb.pose_distance, kb.OfflineKeyframeBuffer.try_new_keyframe,
         kb.OfflineKeyframeBuffer.get_best_measurement_frames_for_0index) = self._saved


def padded(rows, width):
    out = np.full((len(rows), width), -1, np.int32)
    for i, row in enumerate(rows):
        out[i, :len(row)] = row
    return out


def online_keyframes(kb, poses):
    cfg = kb.DVMVS_Config
    gate = kb.KeyframeBuffer(cfg.test_keyframe_buffer_size, cfg.test_keyframe_pose_distance, cfg.test_optimal_t_measure,
                             cfg.test_optimal_R_measure, True)
    return [i for i in range(len(poses)) if gate.try_new_keyframe(poses[i].copy(), None, index=i) == 1]


def main():
    kb, gen = import_generator()
    functions = {"offline": gen.offline_dvmvs_tuples, "dense": gen.dense_dvmvs_tuples,
                 "dense_offline": gen.offline_dense_dvmvs_tuples}
    out = {"margin": np.float64(MARGIN)}
    probe = Probe(kb)
    for name in tc.STREAMS:
        poses = tc.stream(name)
        pose_list = [p for p in poses]
        out[f"{name}_keyframes"] = np.array(online_keyframes(kb, poses), np.int32)
        for mode in tc.MODES:
            for n in tc.measurement_counts(name):
                probe.reset()
                with probe:
                    samples = functions[mode]("scan", pose_list, n)
                key = f"{name}_{mode}_n{n}"
                refs = out[f"{name}_keyframes"].tolist() if mode == "offline" else list(range(len(poses)))
                assert len(probe.ranked) == len(refs)
                out[key] = padded([s["indices"] for s in samples], 1 + n)
                # one row per walk, frame 0's included, sources by (penalty, age in the buffer): walk_tuples' raw output
                out[key + "_ranked"] = padded([[r] + row for r, row in zip(refs, probe.ranked)], 1 + n)
                out[key + "_events"] = np.array([probe.overflows, probe.walks_overflowed, probe.nonlast_rejections], np.int64)
                out[key + "_margins"] = np.array([probe.admission_margin, probe.penalty_margin])
                print(f"{key}: {len(samples)} tuples, {probe.walks_overflowed} walks overflowed, {probe.nonlast_rejections} "
                      f"rejections by a non-last entry, margins {probe.admission_margin:.3g} {probe.penalty_margin:.3g}")
                assert probe.admission_margin >= MARGIN and probe.penalty_margin >= MARGIN, key
                if name == "a":
                    assert probe.walks_overflowed >= 1, key
                    if mode != "dense":
                        assert probe.walks_overflowed == len(refs) and probe.nonlast_rejections >= 1, key
                if name == "b":
                    assert probe.overflows == 0, key
                if name == "c" and mode == "dense":
                    assert probe.nonlast_rejections >= 1, key
    assert any(row[1] == -1 for row in out["a_dense_n7"].tolist()), "no single-index tuple in (a) dense"

    # (e): the buffer classes frame by frame, every return code
    cfg = kb.DVMVS_Config
    poses = tc.lost_pose_stream()
    off = kb.OfflineKeyframeBuffer(cfg.test_keyframe_buffer_size, cfg.test_keyframe_pose_distance, cfg.test_optimal_t_measure,
                                   cfg.test_optimal_R_measure, True)
    simple = kb.SimpleBuffer(7, True)
    codes_off, codes_simple, best_off, best0_off, frames_simple = [], [], [], [], []
    probe.reset()
    with probe:
        for i, pose in enumerate(poses):
            code = off.try_new_keyframe(pose.copy(), None, index=i)
            codes_off.append(code)
            if code == 1:
                probe._scoring = True       # (penalties, not admissions)
                best_off.append([i] + [f[2] for f in off.get_best_measurement_frames(7)])
                probe._scoring = False
                best0_off.append([i] + [f[2] for f in off.get_best_measurement_frames_for_0index(7)])
            code = simple.try_new_keyframe(pose.copy(), None, index=i)
            codes_simple.append(code)
            if code == 1:
                frames_simple.append([i] + [f[2] for f in simple.get_measurement_frames()])
    assert set(codes_off) == {0, 1, 2, 3, 4, 5} and set(codes_simple) == {0, 1, 2, 3, 4}
    assert probe.admission_margin >= MARGIN and probe.penalty_margin >= MARGIN
    out["e_offline_codes"] = np.array(codes_off, np.int8)
    out["e_simple_codes"] = np.array(codes_simple, np.int8)
    out["e_offline_best"] = padded(best_off, 8)
    out["e_offline_best_0index"] = padded(best0_off, 8)
    out["e_simple_frames"] = padded(frames_simple, 8)
    out["e_margins"] = np.array([probe.admission_margin, probe.penalty_margin])
    np.savez_compressed(tc.GOLDEN, **out)
    print("wrote", tc.GOLDEN, os.path.getsize(tc.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
