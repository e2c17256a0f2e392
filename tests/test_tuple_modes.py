"""Host path of the offline / dense / dense_offline tuple modes and of SimpleBuffer / OfflineKeyframeBuffer
(simplerecon_amd.keyframes) against what the reference's generate_test_tuples.py and keyframe_buffer.py gave on the
streams of tests/tuple_cases.py (tests/golden/tuple_modes.npz, recorded by tests/golden/make_tuple_golden.py).
Tuples are compared as (reference frame, SET of sources, count) in tuple order: the reference returns the sources in
np.argpartition's internal order and its dataset sorts them again before use."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tuple_cases as tc
from simplerecon_amd import keyframes as kf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = {"offline": kf.offline_dvmvs_tuples, "dense": kf.dense_dvmvs_tuples,
             "dense_offline": kf.offline_dense_dvmvs_tuples}
CASES = [(s, m, n) for s in tc.STREAMS for m in tc.MODES for n in tc.measurement_counts(s)]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(tc.GOLDEN))


def test_golden_streams_provoke_what_they_are_for(gold):
    """The recorded event counts and margins: every walk of (a) overflows its buffer in the two offline modes, most do in
    dense; (b) never does; (c) makes the backward-only walk meet a rejection by an entry that is not the newest; every
    decision is 1e-9 clear of its threshold."""
    for s, m, n in CASES:
        overflows, walks_overflowed, nonlast = gold[f"{s}_{m}_n{n}_events"].tolist()
        assert (gold[f"{s}_{m}_n{n}_margins"] >= gold["margin"]).all()
        if s == "a":
            walks = len(gold[f"{s}_{m}_n{n}_ranked"])
            assert walks_overflowed == walks if m != "dense" else 1 <= walks_overflowed < walks
            assert (nonlast >= 1) == (m != "dense")
        if s == "b":
            assert overflows == 0
        if (s, m) == ("c", "dense"):
            assert nonlast >= 1
    assert [len(gold[f"a_{m}_n7"]) for m in tc.MODES] == [188, 219, 220]
    assert gold["a_dense_n7"][0].tolist() == [1] + [-1] * 7        # a tuple of one index is kept for frame 1
    assert gold["a_dense_n40"].max(axis=0)[29] == -1 and (gold["a_dense_n40"][:, 28] >= 0).any()   # 28 is all dense has


@pytest.mark.parametrize("stream,mode,n", CASES)
def test_host_tuples_match_the_reference(gold, stream, mode, n):
    poses = tc.stream(stream)
    samples = FUNCTIONS[mode]("scan", [p for p in poses], n)
    assert all(s["scan"] == "scan" and set(s) == {"scan", "indices"} for s in samples)
    assert tc.tuples_as_comparable(samples) == tc.rows_as_comparable(gold[f"{stream}_{mode}_n{n}"])
    assert all(isinstance(i, (int, np.integer)) for s in samples for i in s["indices"])


def test_poses_are_taken_as_arrays_lists_and_fp32(gold):
    """An [N,4,4] array, a list and a tensor give the same tuples; fp32 poses are converted to fp64 first."""
    import torch
    poses = tc.stream("b")
    want = tc.rows_as_comparable(gold["b_dense_offline_n7"])
    assert tc.tuples_as_comparable(kf.offline_dense_dvmvs_tuples("s", poses, 7)) == want
    assert tc.tuples_as_comparable(kf.offline_dense_dvmvs_tuples("s", torch.from_numpy(poses), 7)) == want
    f32 = poses.astype(np.float32)
    assert (tc.tuples_as_comparable(kf.dense_dvmvs_tuples("s", f32, 7))
            == tc.tuples_as_comparable(kf.dense_dvmvs_tuples("s", f32.astype(np.float64), 7)))


def test_compute_offline_tuple_matches_the_reference(gold):
    poses = tc.stream("a")
    rows = tc.rows_as_comparable(gold["a_dense_offline_n7"])
    for i in (0, 1, 57, 100, 219):
        sample = kf.compute_offline_tuple(poses, 7, i, poses[i])
        assert set(sample) == {"indices"} and tc.tuples_as_comparable([sample]) == [rows[i]]


def test_offline_keyframes_are_the_online_buffers(gold):
    for s in tc.STREAMS:
        assert kf._online_keyframes(tc.stream(s)) == gold[f"{s}_keyframes"].tolist()
    assert 0 < len(gold["a_keyframes"]) < 220


def test_buffer_classes_frame_by_frame(gold):
    """(e): poses go missing for short and for long stretches; every return code of both classes, and what the buffers
    hold, as the reference's."""
    cfg = kf.DVMVS_Config
    off = kf.OfflineKeyframeBuffer(cfg.test_keyframe_buffer_size, cfg.test_keyframe_pose_distance,
                                   cfg.test_optimal_t_measure, cfg.test_optimal_R_measure, store_return_indices=True)
    simple = kf.SimpleBuffer(7, store_return_indices=True)
    codes_off, codes_simple, best, best0, frames = [], [], [], [], []
    for i, pose in enumerate(tc.lost_pose_stream()):
        code = off.try_new_keyframe(pose, None, index=i)
        codes_off.append(code)
        if code == off.ADDED:
            best.append({"indices": [i] + [f[2] for f in off.get_best_measurement_frames(7)]})
            best0.append({"indices": [i] + [f[2] for f in off.get_best_measurement_frames_for_0index(7)]})
        code = simple.try_new_keyframe(pose, None, index=i)
        codes_simple.append(code)
        if code == simple.ADDED:
            frames.append([i] + [f[2] for f in simple.get_measurement_frames()])
        assert len(off.buffer) <= cfg.test_keyframe_buffer_size and len(simple.buffer) <= 8
    assert np.array_equal(np.array(codes_off, np.int8), gold["e_offline_codes"])
    assert np.array_equal(np.array(codes_simple, np.int8), gold["e_simple_codes"])
    assert set(codes_off) == {0, 1, 2, 3, 4, 5} and set(codes_simple) == {0, 1, 2, 3, 4}
    assert tc.tuples_as_comparable(best) == tc.rows_as_comparable(gold["e_offline_best"])
    assert tc.tuples_as_comparable(best0) == tc.rows_as_comparable(gold["e_offline_best_0index"])
    want = [[v for v in row if v >= 0] for row in gold["e_simple_frames"].tolist()]
    assert frames == want                                  # SimpleBuffer keeps its frames in order


def test_buffer_classes_constructor_and_index_rule():
    off = kf.OfflineKeyframeBuffer(buffer_size=3, keyframe_pose_distance=0.1, optimal_t_score=0.15, optimal_R_score=0.0,
                                   store_return_indices=False)
    assert off.buffer.maxlen == 3 and kf.SimpleBuffer(buffer_size=3, store_return_indices=True).buffer.maxlen == 4
    assert off.try_new_keyframe(np.eye(4), "image") == 0 and off.buffer[0][1] == "image" and len(off.buffer[0]) == 2
    assert off.get_best_measurement_frames_for_0index(7) == []
    assert off.calculate_penalty(0.05, 0.0) == pytest.approx(5 * 0.1 ** 2) and off.calculate_penalty(0.25, 0.1) == pytest.approx(0.02)
    for buf in (kf.OfflineKeyframeBuffer(3, 0.1, 0.15, 0.0, True), kf.SimpleBuffer(3, True)):
        with pytest.raises(ValueError):
            buf.try_new_keyframe(np.eye(4), None)


def test_tuple_file_of_the_dense_offline_mode(gold, tmp_path):
    samples = kf.offline_dense_dvmvs_tuples("scene0707_00", tc.stream("a"), 7)
    path = tmp_path / "tuples.txt"
    kf.write_tuple_file(str(path), samples)
    lines = path.read_text().splitlines()
    assert len(lines) == 220 and all(len(line.split()) == 9 and line.split()[0] == "scene0707_00" for line in lines)
    got = [{"indices": [int(v) for v in line.split()[1:]]} for line in lines]
    assert tc.tuples_as_comparable(got) == tc.rows_as_comparable(gold["a_dense_offline_n7"])


def test_make_tuples_example_end_to_end(gold, tmp_path):
    """examples/make_tuples.py on stream (b), host path (--device omitted): `scan id0 id1 ...` lines, the golden tuples."""
    np.save(tmp_path / "scan.npy", tc.stream("b"))
    out = tmp_path / "dense_offline.txt"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "make_tuples.py"), "--poses", str(tmp_path / "scan.npy"),
                          "--mode", "dense_offline", "--num-images-in-tuple", "8", "--scan", "scene_b", "--out", str(out)],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = out.read_text().splitlines()
    assert all(line.split()[0] == "scene_b" for line in lines)
    got = [{"indices": [int(v) for v in line.split()[1:]]} for line in lines]
    assert tc.tuples_as_comparable(got) == tc.rows_as_comparable(gold["b_dense_offline_n7"])


def test_device_path_refuses_bad_poses_before_it_touches_a_device():
    """The pose checks of the device path are host code: a frame without a pose, or a bottom row other than 0 0 0 1,
    raises ValueError naming the frame (device=None, the host path, takes both)."""
    poses = tc.stream("b")
    bad = poses.copy()
    bad[17, 1, 2] = np.nan
    with pytest.raises(ValueError, match="frame 17"):
        kf.dense_dvmvs_tuples("s", bad, 7, device="cuda")
    bad = poses.copy()
    bad[5, 3, 3] = 2.0
    with pytest.raises(ValueError, match="frame 5"):
        kf.offline_dense_dvmvs_tuples("s", bad, 7, device="cuda")
    kf.check_walk_poses(poses)
