"""Device path of the offline / dense / dense_offline tuple modes (csrc/sr_tuples.hip through simplerecon_amd.keyframes)
against the reference's recorded tuples (tests/golden/tuple_modes.npz) and against the host path."""
import numpy as np
import pytest
import torch

import tuple_cases as tc
from simplerecon_amd import _lib
from simplerecon_amd import keyframes as kf

pytestmark = pytest.mark.gpu
DEV = "cuda"
FUNCTIONS = {"offline": kf.offline_dvmvs_tuples, "dense": kf.dense_dvmvs_tuples,
             "dense_offline": kf.offline_dense_dvmvs_tuples}
CASES = [(s, m, n) for s in tc.STREAMS for m in tc.MODES for n in tc.measurement_counts(s)]
RANDOM_SEED = 12       # a seed for which both margins of the 300-frame stream hold (searched on the CPU: 4e-4 and 1e-4)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(tc.GOLDEN))


def _walk(poses, refs, n, mode, **kw):
    both = mode != "dense"
    return kf.walk_tuples(torch.from_numpy(poses).to(DEV), torch.tensor(list(refs), dtype=torch.int32, device=DEV), n, both,
                          60 if both else 30, **kw)


def test_pose_inverse_is_a_general_inverse():
    poses = tc.stream("a")
    rng = np.random.default_rng(0)
    skewed = poses + rng.normal(0.0, 1e-3, poses.shape)            # not rigid, bottom row not 0 0 0 1
    for p in (poses, skewed, np.zeros((0, 4, 4))):
        got = kf.pose_inverse(torch.from_numpy(p).to(DEV)).cpu().numpy()
        want = np.linalg.inv(p) if len(p) else p
        # both inverses are backward stable; cond <= ~100 here (|t| <= 2.5), eps = 1.1e-16
        assert got.shape == want.shape and np.abs(got - want).max(initial=0.0) <= 1e-12


@pytest.mark.parametrize("stream,mode,n", CASES)
def test_device_tuples_match_the_reference(gold, stream, mode, n):
    samples = FUNCTIONS[mode]("scan", [p for p in tc.stream(stream)], n, device=DEV)
    assert all(s["scan"] == "scan" and set(s) == {"scan", "indices"} for s in samples)
    assert all(type(i) is int for s in samples for i in s["indices"])
    assert tc.tuples_as_comparable(samples) == tc.rows_as_comparable(gold[f"{stream}_{mode}_n{n}"])


@pytest.mark.parametrize("stream,mode,n", CASES)
def test_walk_tuples_raw_output(gold, stream, mode, n):
    """indices: the reference frame, the sources by ascending penalty (ties by age in the buffer), -1 to the end of the
    row; counts: the number of sources.  The offline mode hands in a strict subset of the frames as reference list, which
    a kernel that indexed by row instead of by reference index would get wrong."""
    poses = tc.stream(stream)
    want = gold[f"{stream}_{mode}_n{n}_ranked"]
    refs = gold[f"{stream}_keyframes"].tolist() if mode == "offline" else range(len(poses))
    if stream == "a" and mode == "offline":
        assert 0 < len(refs) < len(poses) and refs != list(range(len(refs)))
    indices, counts = _walk(poses, refs, n, mode)
    assert indices.dtype == torch.int32 and counts.dtype == torch.int32 and indices.is_cuda and counts.is_cuda
    assert tuple(indices.shape) == (len(want), 1 + n) and tuple(counts.shape) == (len(want),)
    assert np.array_equal(indices.cpu().numpy(), want)
    assert np.array_equal(counts.cpu().numpy(), (want[:, 1:] >= 0).sum(axis=1))


def test_device_matches_host_on_a_random_stream():
    """A further 300-frame stream with stretches where the camera almost rests.  First the two conditions on the input
    (host code): every admission distance and every source choice 1e-9 clear of its threshold."""
    poses = tc.random_stream(300, RANDOM_SEED)
    with tc.HostMargins(kf) as margins:
        host = {m: FUNCTIONS[m]("s", poses, 7) for m in ("dense_offline", "dense")}
    print(f"margins: admission {margins.admission:.3g}, penalty {margins.penalty:.3g}")
    assert margins.admission >= 1e-9 and margins.penalty >= 1e-9
    for m, want in host.items():
        got = FUNCTIONS[m]("s", poses, 7, device=DEV)
        assert tc.tuples_as_comparable(got) == tc.tuples_as_comparable(want), m
    # the offline mode walks from the online keyframes only: the same walks as dense_offline's at those frames
    keyframes = kf._online_keyframes(poses)
    by_frame = {s["indices"][0]: s for s in host["dense_offline"]}
    assert 0 < len(keyframes) < 300
    assert (tc.tuples_as_comparable(kf.offline_dvmvs_tuples("s", poses, 7, device=DEV))
            == tc.tuples_as_comparable([by_frame[i] for i in keyframes]))


def test_the_same_call_twice_gives_the_same_bytes():
    poses = tc.stream("a")
    for mode in ("dense_offline", "dense"):
        a = [t.cpu().numpy().tobytes() for t in _walk(poses, range(220), 7, mode)]
        b = [t.cpu().numpy().tobytes() for t in _walk(poses, range(220), 7, mode)]
        assert a == b


def test_empty_inputs():
    poses = tc.stream("b")
    indices, counts = _walk(poses, [], 7, "dense")                                    # M = 0
    assert tuple(indices.shape) == (0, 8) and tuple(counts.shape) == (0,)
    indices, counts = _walk(np.zeros((0, 4, 4)), [], 7, "dense_offline")              # N = 0
    assert tuple(indices.shape) == (0, 8) and tuple(counts.shape) == (0,)
    for mode in tc.MODES:
        assert FUNCTIONS[mode]("s", [], 7, device=DEV) == []
    # a reference index that is no frame of the scan: an empty row, no read
    indices, counts = _walk(poses, [48, -1, 3], 7, "dense_offline")
    assert indices[:2].cpu().tolist() == [[-1] * 8] * 2 and counts.cpu().tolist()[:2] == [0, 0] and indices[2, 0].item() == 3
    indices, counts = _walk(poses, [5], 0, "dense")                                   # no sources asked for
    assert indices.cpu().tolist() == [[5]] and counts.cpu().tolist() == [0]


def test_refusals():
    poses = tc.stream("b")
    bad = poses.copy()
    bad[17, 0, 3] = np.nan
    with pytest.raises(ValueError, match="frame 17"):
        kf.offline_dense_dvmvs_tuples("s", bad, 7, device=DEV)
    bad = poses.copy()
    bad[5, 3] = [0.0, 0.0, 0.0, 2.0]
    with pytest.raises(ValueError, match="frame 5"):
        kf.dense_dvmvs_tuples("s", bad, 7, device=DEV)
    dev_poses = torch.from_numpy(poses).to(DEV)
    refs = torch.arange(48, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.HipLibraryError, match="unsupported"):
        kf.walk_tuples(dev_poses, refs, 7, True, 65)
    with pytest.raises(_lib.HipLibraryError, match="unsupported"):
        kf.walk_tuples(dev_poses, refs, 64, True, 60)
    with pytest.raises(_lib.HipLibraryError, match="cpu"):
        kf.walk_tuples(torch.from_numpy(poses), refs, 7, True, 60)
    with pytest.raises(_lib.HipLibraryError):
        kf.walk_tuples(dev_poses, refs.cpu(), 7, True, 60)
    with pytest.raises(_lib.HipLibraryError):
        kf.dense_dvmvs_tuples("s", poses, 7, device="cpu")
    with pytest.raises(TypeError):
        kf.walk_tuples(dev_poses.float(), refs, 7, True, 60)
    # the C ABI itself: NULL and misaligned pointers
    lib, stream = _lib.lib(), _lib.stream_ptr(dev_poses.device)
    inv = kf.pose_inverse(dev_poses)
    out, cnt = torch.empty((48, 8), dtype=torch.int32, device=DEV), torch.empty(48, dtype=torch.int32, device=DEV)

    def call(p=dev_poses.data_ptr(), i=inv.data_ptr(), r=refs.data_ptr(), o=out.data_ptr(), c=cnt.data_ptr(), size=60, n=7):
        return lib.sr_tuple_walk_f64(p, i, 48, r, 48, 1, size, size, 0.1, 0.15, 0.0, n, o, c, stream)
    assert call(p=None) == 1 and call(o=None) == 1 and call(r=None) == 1
    assert call(p=dev_poses.data_ptr() + 4) == 1 and call(c=cnt.data_ptr() + 2) == 1 and call(size=0) == 1
    assert call(size=65) == _lib.ERR_UNSUPPORTED and call(n=64) == _lib.ERR_UNSUPPORTED
    assert lib.sr_pose_inverse_f64(None, inv.data_ptr(), 3, stream) == 1
    assert lib.sr_pose_inverse_f64(dev_poses.data_ptr() + 4, inv.data_ptr(), 3, stream) == 1
    assert call() == 0
    torch.cuda.synchronize()
