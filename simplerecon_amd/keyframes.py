"""Online keyframe / source-view selection in front of the depth hot path -- the streaming counterpart of the
precomputed test tuples (SURVEY.md §8f "next" #4).  API-compatible with the reference's tools/keyframe_buffer.py
(`KeyframeBuffer`, `DVMVS_Config`, `pose_distance`; DeepVideoMVS heuristics) and with the source ordering of
datasets/generic_mvs_dataset.py:643-659.  The online buffer is host-side control logic on numpy, like the reference's: one
buffer fed one pose at a time is a handful of 4x4 operations per frame and stays on the host.

    buf = KeyframeBuffer(DVMVS_Config.test_keyframe_buffer_size, DVMVS_Config.test_keyframe_pose_distance,
                         DVMVS_Config.test_optimal_t_measure, DVMVS_Config.test_optimal_R_measure, store_return_indices=True)
    if buf.try_new_keyframe(world_T_cam, image, index=i) == KeyframeBuffer.ADDED:
        sources = buf.get_best_measurement_frames(7)      # [(pose, image, index), ...]

The tuple files of a scan come from the four modes of the reference's data_scripts/generate_test_tuples.py:
`default_dvmvs_tuples` (online), `offline_dvmvs_tuples`, `dense_dvmvs_tuples` and `offline_dense_dvmvs_tuples`, on
`SimpleBuffer` / `OfflineKeyframeBuffer` / `compute_offline_tuple` (keyframe_buffer.py:189-381).  The last three start an
independent walk over the scan from every (key)frame, each step of which tests one pose against a buffer of up to 60: with
`device=None` they run on the host like the reference, with a CUDA device the walks run one wave per frame
(csrc/sr_tuples.hip, `walk_tuples`) and the same list of dictionaries comes back after one device-to-host copy.

    samples = offline_dense_dvmvs_tuples("scene0707_00", poses, 7, device="cuda")
    write_tuple_file("test_eight_view_deepvmvs_dense_offline.txt", samples)

All of it computes in fp64: poses are converted on entry.  The reference computes in whatever dtype its loader hands it;
for fp32 poses its decisions can differ from these where a pose distance lies within fp32 rounding of a threshold.
"""
import collections

import numpy as np


class DVMVS_Config:
    """Tuple settings of the reference (tools/keyframe_buffer.py:12-22)."""
    train_minimum_pose_distance = 0.125
    train_maximum_pose_distance = 0.325
    train_crawl_step = 3
    test_keyframe_buffer_size = 30
    test_keyframe_pose_distance = 0.1
    test_optimal_t_measure = 0.15
    test_optimal_R_measure = 0.0


def is_pose_available(pose):
    """False when tracking delivered NaN / inf (keyframe_buffer.py:24-31)."""
    return bool(np.isfinite(pose).all())


def pose_distance(reference_pose, measurement_pose):
    """DVMVS pose measures between two camera-to-world poses (keyframe_buffer.py:53-69):
    returns (combined, R_measure, t_measure) with R = sqrt(2 (1 - min(3, tr R) / 3)), t = |t|."""
    return _pose_measures(np.linalg.inv(reference_pose), measurement_pose)


def _pose_measures(inverse_reference_pose, measurement_pose):
    """pose_distance() behind the inverse: the walks test one pose against a whole buffer and invert it once."""
    rel = np.dot(inverse_reference_pose, measurement_pose)
    R_measure = np.sqrt(2 * (1 - min(3.0, np.trace(rel[:3, :3])) / 3))
    t_measure = np.linalg.norm(rel[:3, 3])
    return np.sqrt(t_measure ** 2 + R_measure ** 2), R_measure, t_measure


def is_valid_pair(reference_pose, measurement_pose, pose_dist_min, pose_dist_max, t_norm_threshold=0.05,
                  return_measure=False):
    """Training-tuple validity test (keyframe_buffer.py:33-51)."""
    combined, _, t_measure = pose_distance(reference_pose, measurement_pose)
    ok = bool(pose_dist_min <= combined <= pose_dist_max and t_measure >= t_norm_threshold)
    return (ok, combined) if return_measure else ok


class KeyframeBuffer:
    """Bounded FIFO of keyframes with the DVMVS admission rule and source-view choice (keyframe_buffer.py:71-186).

    try_new_keyframe() return codes (the reference's): 0 first frame stored, 1 new keyframe stored (predict depth),
    2 not enough motion, 3 buffer reset (tracking lost / gap in valid frames), 4 still lost, 5 pose missing (waiting)."""
    FIRST, ADDED, TOO_CLOSE, RESET, LOST, WAITING = 0, 1, 2, 3, 4, 5
    LOST_AFTER = 30  # frames without a pose (about a second) before the buffer is dropped

    def __init__(self, buffer_size, keyframe_pose_distance, optimal_t_score, optimal_R_score, store_return_indices):
        self.buffer_size = buffer_size
        self.keyframe_pose_distance = keyframe_pose_distance
        self.optimal_t_score = optimal_t_score
        self.optimal_R_score = optimal_R_score
        self._with_index = store_return_indices
        self._frames = []          # oldest first; entries (pose, image[, index])
        self._missing = 0

    # the reference exposes its deque as `.buffer`
    @property
    def buffer(self):
        return self._frames

    def _push(self, pose, image, index):
        self._frames.append((pose, image, index) if self._with_index else (pose, image))
        if len(self._frames) > self.buffer_size:
            del self._frames[0]

    def calculate_penalty(self, t_score, R_score):
        """Squared distance from the optimal baseline; too-short baselines cost 5x (keyframe_buffer.py:90-98)."""
        t_diff = t_score - self.optimal_t_score
        t_penalty = (5.0 if t_diff < 0.0 else 1.0) * np.abs(t_diff) ** 2.0
        return np.abs(R_score - self.optimal_R_score) ** 2.0 + t_penalty

    def try_new_keyframe(self, pose, image, dist_to_last_valid=None, index=None):
        if self._with_index and index is None:
            raise ValueError("Storing and returning the frame indices is requested in the constructor, but "
                             "index=None is passed to the function")
        if dist_to_last_valid is not None and dist_to_last_valid > 30:   # gap in the valid-frame list
            self._frames.clear()
            self._missing = 0
            self._push(pose, image, index)
            return self.RESET
        if not is_pose_available(pose):
            self._missing += 1
            if self._missing <= self.LOST_AFTER:
                return self.WAITING
            if self._frames:
                self._frames.clear()
                return self.RESET
            return self.LOST
        self._missing = 0
        if not self._frames:
            self._push(pose, image, index)
            return self.FIRST
        combined, _, _ = pose_distance(pose, self._frames[-1][0])
        if combined >= self.keyframe_pose_distance:
            self._push(pose, image, index)
            return self.ADDED
        return self.TOO_CLOSE

    def get_best_measurement_frames(self, n_requested_measurement_frames):
        """The n buffered frames whose baseline to the newest keyframe is closest to the optimum (unordered, as
        np.argpartition returns them -- the dataset orders sources afterwards, see sort_sources_by_pose_penalty)."""
        reference_pose = self._frames[-1][0]
        candidates = self._frames[:-1]
        n = min(n_requested_measurement_frames, len(candidates))
        penalties = []
        for frame in candidates:
            _, R_measure, t_measure = pose_distance(reference_pose, frame[0])
            penalties.append(self.calculate_penalty(t_measure, R_measure))
        chosen = np.argpartition(penalties, n - 1)[:n]
        return [candidates[i] for i in chosen]


def default_dvmvs_tuples(scan, poses, dists_to_last_valid, n_measurement_frames):
    """The reference's default ("online") test tuples for one scan -- the list its evaluation runs on
    (data_scripts/generate_test_tuples.py:159-212): every pose is offered to a KeyframeBuffer with the DVMVS test
    settings; each accepted keyframe yields {"scan": scan, "indices": [keyframe, source, ...]} with up to
    n_measurement_frames earlier keyframes chosen by baseline penalty.  `dists_to_last_valid[i]` = frames since the
    last valid pose (None to let the buffer handle invalid poses itself)."""
    cfg = DVMVS_Config
    buf = KeyframeBuffer(cfg.test_keyframe_buffer_size, cfg.test_keyframe_pose_distance, cfg.test_optimal_t_measure,
                         cfg.test_optimal_R_measure, store_return_indices=True)
    samples = []
    for i, pose in enumerate(poses):
        if buf.try_new_keyframe(np.array(pose, copy=True), None, dists_to_last_valid[i], index=i) != buf.ADDED:
            continue
        sources = [frame[2] for frame in buf.get_best_measurement_frames(n_measurement_frames)]
        samples.append({"scan": scan, "indices": [i] + sources})
    return samples


class _LostPoseCounter:
    """What SimpleBuffer and OfflineKeyframeBuffer do with a pose that tracking did not deliver: wait for LOST_AFTER
    frames, then drop the buffer once and report `lost` until a pose arrives (keyframe_buffer.py:224-239, 315-330)."""
    LOST_AFTER = 30

    def __init__(self, buffer_size):
        self.buffer = collections.deque([], maxlen=buffer_size)   # oldest first, as the reference exposes it
        self._missing = 0

    def _missing_pose(self, reset, lost, waiting):
        self._missing += 1
        if self._missing <= self.LOST_AFTER:
            return waiting
        if self.buffer:
            self.buffer.clear()
            return reset
        return lost

    def _entry(self, pose, image, index):
        if self._with_index and index is None:
            raise ValueError("Storing and returning the frame indices is requested in the constructor, but "
                             "index=None is passed to the function")
        return (pose, image, index) if self._with_index else (pose, image)


class SimpleBuffer(_LostPoseCounter):
    """Keeps every frame that has a pose: the last `buffer_size` of them are the sources of the newest
    (keyframe_buffer.py:189-243).  try_new_keyframe() returns 0 first frame, 1 frame stored, 2 buffer dropped (tracking
    lost), 3 still lost, 4 pose missing (waiting)."""
    FIRST, ADDED, RESET, LOST, WAITING = 0, 1, 2, 3, 4

    def __init__(self, buffer_size, store_return_indices):
        super().__init__(buffer_size + 1)
        self._with_index = store_return_indices

    def try_new_keyframe(self, pose, image, index=None):
        entry = self._entry(pose, image, index)
        if not is_pose_available(pose):
            return self._missing_pose(self.RESET, self.LOST, self.WAITING)
        self._missing = 0
        code = self.ADDED if self.buffer else self.FIRST
        self.buffer.append(entry)
        return code

    def get_measurement_frames(self):
        return list(self.buffer)[:-1]


class OfflineKeyframeBuffer(_LostPoseCounter):
    """The buffer of the offline and dense walks (keyframe_buffer.py:245-381): a pose is admitted when its distance to
    EVERY buffered pose reaches the keyframe distance, not only to the newest.  Return codes as KeyframeBuffer's (there is
    no valid-frame gap here, so 3 only follows lost tracking).  A full buffer loses its oldest entry to a new one."""
    FIRST, ADDED, TOO_CLOSE, RESET, LOST, WAITING = 0, 1, 2, 3, 4, 5

    def __init__(self, buffer_size, keyframe_pose_distance, optimal_t_score, optimal_R_score, store_return_indices):
        super().__init__(buffer_size)
        self.keyframe_pose_distance = keyframe_pose_distance
        self.optimal_t_score = optimal_t_score
        self.optimal_R_score = optimal_R_score
        self._with_index = store_return_indices

    calculate_penalty = KeyframeBuffer.calculate_penalty

    def try_new_keyframe(self, pose, image, index=None):
        entry = self._entry(pose, image, index)
        if not is_pose_available(pose):
            return self._missing_pose(self.RESET, self.LOST, self.WAITING)
        self._missing = 0
        if not self.buffer:
            self.buffer.append(entry)
            return self.FIRST
        inverse = np.linalg.inv(pose)
        for frame in self.buffer:
            if _pose_measures(inverse, frame[0])[0] < self.keyframe_pose_distance:
                return self.TOO_CLOSE
        self.buffer.append(entry)
        return self.ADDED

    def _best(self, reference_pose, candidates, n):
        inverse = np.linalg.inv(reference_pose)
        penalties = []
        for frame in candidates:
            _, R_measure, t_measure = _pose_measures(inverse, frame[0])
            penalties.append(self.calculate_penalty(t_measure, R_measure))
        chosen = np.argpartition(penalties, n - 1)[:n]
        return [candidates[i] for i in chosen]

    def get_best_measurement_frames(self, n_requested_measurement_frames):
        """As KeyframeBuffer's: the newest entry is the reference, the others are scored."""
        frames = list(self.buffer)
        return self._best(frames[-1][0], frames[:-1], min(n_requested_measurement_frames, len(frames) - 1))

    def get_best_measurement_frames_for_0index(self, n_requested_measurement_frames):
        """The sources of a walk that was primed with its reference frame (keyframe_buffer.py:357-381), with the
        reference's arithmetic as it stands: the OLDEST entry is dropped -- the primed frame only until a full buffer has
        pushed it out --, the next one serves as the reference pose of the penalties and is scored against itself with
        the others (penalty 5 optimal_t^2, and it can be chosen), and min(n, entries left - 1) frames are returned."""
        frames = list(self.buffer)[1:]
        if not frames:
            return []
        return self._best(frames[0][0], frames, min(n_requested_measurement_frames, len(frames) - 1))


def _poses_f64(poses):
    """[N,4,4] float64 from a list of 4x4 arrays, an array or a tensor (the arithmetic of every tuple mode)."""
    if hasattr(poses, "detach"):
        poses = poses.detach().cpu().numpy()
    return np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)


def _offline_buffer(buffer_size):
    cfg = DVMVS_Config
    return OfflineKeyframeBuffer(buffer_size, cfg.test_keyframe_pose_distance, cfg.test_optimal_t_measure,
                                 cfg.test_optimal_R_measure, store_return_indices=True)


def compute_offline_tuple(poses, n_measurement_frames, current_keyframe_index, reference_pose):
    """One offline tuple (generate_test_tuples.py:65-157): a buffer of 2 x 30 primed with the reference pose is offered
    the frames after and before it in turn, forward first -- a direction that has run out still takes its turn --, until
    both have run out or 60 frames were admitted.  The 60th admission pushes the primed frame out of the full buffer;
    get_best_measurement_frames_for_0index() then chooses among what is left.  Returns {"indices": [frame, source, ...]}."""
    size = DVMVS_Config.test_keyframe_buffer_size * 2
    buf = _offline_buffer(size)
    buf.try_new_keyframe(np.array(reference_pose, copy=True), None, index=current_keyframe_index)
    following, preceding = current_keyframe_index + 1, current_keyframe_index - 1
    forward, added = True, 0
    forward_left = backward_left = True
    while forward_left or backward_left:
        if forward:
            forward = False
            if following >= len(poses):
                forward_left = False
                continue
            candidate = following
            following += 1
        else:
            forward = True
            if preceding < 0:
                backward_left = False
                continue
            candidate = preceding
            preceding -= 1
        if buf.try_new_keyframe(np.array(poses[candidate], copy=True), None, index=candidate) == buf.ADDED:
            added += 1
        if added >= size:
            break
    sources = buf.get_best_measurement_frames_for_0index(n_measurement_frames)
    return {"indices": [current_keyframe_index] + [frame[2] for frame in sources]}


def _keep(sample, frame):
    """Only the first frame of a scan is dropped for having no sources (generate_test_tuples.py:261-265): a later frame
    whose walk found none is written as a tuple of one index."""
    return not (len(sample["indices"]) == 1 and frame == 0)


def _online_keyframes(poses):
    """Frames an online KeyframeBuffer with the DVMVS test settings accepts as new keyframes (never frame 0)."""
    cfg = DVMVS_Config
    gate = KeyframeBuffer(cfg.test_keyframe_buffer_size, cfg.test_keyframe_pose_distance, cfg.test_optimal_t_measure,
                          cfg.test_optimal_R_measure, store_return_indices=True)
    return [i for i, pose in enumerate(poses) if gate.try_new_keyframe(pose, None, index=i) == gate.ADDED]


def offline_dvmvs_tuples(scan, poses, n_measurement_frames, device=None):
    """The reference's "offline" tuples of one scan (generate_test_tuples.py:214-266): one compute_offline_tuple() for
    every keyframe of the online buffer, with sources from both sides of it in time.  [{"scan", "indices"}, ...].
    device: None for the host path; a CUDA device runs the walks there (the keyframe gate, N distances, stays on the
    host) and returns the same tuples, the sources in penalty order instead of np.argpartition's."""
    poses = _poses_f64(poses)
    keyframes = _online_keyframes(poses)
    if device is not None:
        return _device_tuples(scan, poses, keyframes, n_measurement_frames, True, device)
    samples = []
    for i in keyframes:
        sample = compute_offline_tuple(poses, n_measurement_frames, i, poses[i])
        sample["scan"] = scan
        if _keep(sample, i):
            samples.append(sample)
    return samples


def dense_dvmvs_tuples(scan, poses, n_measurement_frames, device=None):
    """The reference's "dense" tuples (generate_test_tuples.py:268-343): an online tuple for EVERY frame.  A buffer of 30
    primed with the frame is offered the frames before it, newest first, until the start of the scan or 30 admissions
    (the loop's own condition never changes), the 30th pushing the primed frame out.  Frame 0 has no tuple; a later frame
    without sources has a tuple of one index.  device: as offline_dvmvs_tuples."""
    poses = _poses_f64(poses)
    if device is not None:
        return _device_tuples(scan, poses, range(len(poses)), n_measurement_frames, False, device)
    samples = []
    for i in range(len(poses)):
        sample = _dense_tuple(poses, n_measurement_frames, i)
        sample["scan"] = scan
        if _keep(sample, i):
            samples.append(sample)
    return samples


def _dense_tuple(poses, n_measurement_frames, i):
    """The backward-only walk of dense_dvmvs_tuples for frame i: {"indices": [i, source, ...]}."""
    size = DVMVS_Config.test_keyframe_buffer_size
    buf = _offline_buffer(size)
    buf.try_new_keyframe(poses[i], None, index=i)
    added = 0
    for candidate in range(i - 1, -1, -1) if n_measurement_frames != 0 else ():
        if buf.try_new_keyframe(poses[candidate], None, index=candidate) == buf.ADDED:
            added += 1
        if added >= size:
            break
    sources = buf.get_best_measurement_frames_for_0index(n_measurement_frames)
    return {"indices": [i] + [frame[2] for frame in sources]}


def offline_dense_dvmvs_tuples(scan, poses, n_measurement_frames, device=None):
    """The reference's "dense_offline" tuples (generate_test_tuples.py:345-382): compute_offline_tuple() for EVERY frame.
    device: as offline_dvmvs_tuples."""
    poses = _poses_f64(poses)
    if device is not None:
        return _device_tuples(scan, poses, range(len(poses)), n_measurement_frames, True, device)
    samples = []
    for i in range(len(poses)):
        sample = compute_offline_tuple(poses, n_measurement_frames, i, poses[i])
        sample["scan"] = scan
        if _keep(sample, i):
            samples.append(sample)
    return samples


# ---- device path: csrc/sr_tuples.hip ------------------------------------------------------------------------------------
def check_walk_poses(poses):
    """What the walk kernel requires of its [N,4,4] poses (a host array): finite, bottom row exactly 0 0 0 1 -- it reads
    rows 0..2 only.  Tuple files are built over a scan's valid frames, as the reference's crawl does; a frame without a
    pose raises ValueError here, there is no silent switch to the host path (whose buffers count lost poses)."""
    bad = ~np.isfinite(poses).all(axis=(1, 2))
    if bad.any():
        raise ValueError(f"frame {int(np.argmax(bad))}: the pose is not finite; the device path takes valid frames only")
    bad = (poses[:, 3, :] != np.array([0.0, 0.0, 0.0, 1.0])).any(axis=1)
    if bad.any():
        i = int(np.argmax(bad))
        raise ValueError(f"frame {i}: the pose's bottom row is {poses[i, 3].tolist()}, not 0 0 0 1")


def _device_f64_poses(poses, device):
    import torch
    from . import _lib
    if not isinstance(poses, torch.Tensor):
        raise TypeError(f"poses must be a torch.Tensor, got {type(poses)}")
    if not poses.is_cuda:
        raise _lib.HipLibraryError(f"poses live on {poses.device}: the walk kernel needs device tensors (no CPU fallback)")
    if device is not None:
        device = torch.device(device)
        if device.type != "cuda" or device.index not in (None, poses.device.index):
            raise _lib.HipLibraryError(f"poses live on {poses.device}, the walk was asked for on {device}")
    if poses.dtype != torch.float64 or poses.dim() != 3 or tuple(poses.shape[1:]) != (4, 4):
        raise TypeError(f"poses must be [N,4,4] float64, got {tuple(poses.shape)} {poses.dtype}")
    return poses.contiguous()


def pose_inverse(poses):
    """inv() of [N,4,4] fp64 device poses: a general inverse (tracker poses are not exactly orthonormal)."""
    import torch
    from . import _lib
    poses = _device_f64_poses(poses, None)
    out = torch.empty_like(poses)
    _lib.call("sr_pose_inverse_f64", poses.device, poses, out, poses.shape[0])
    return out


def walk_tuples(poses, reference_indices, n_measurement_frames, both_directions, buffer_size, acceptance_cap=None,
                keyframe_pose_distance=DVMVS_Config.test_keyframe_pose_distance,
                optimal_t=DVMVS_Config.test_optimal_t_measure, optimal_R=DVMVS_Config.test_optimal_R_measure, device=None):
    """The walks of the offline / dense tuple modes on the GPU, one wave per reference frame.  poses [N,4,4] float64 and
    reference_indices [M] int32, both on the device (check_walk_poses() is the caller's: nothing here reads a pose on the
    host).  both_directions: True walks r+1, r-1, r+2, ... (compute_offline_tuple: buffer_size 60), False r-1, r-2, ...
    (dense: 30); acceptance_cap defaults to buffer_size, as in both.  Returns (indices [M, 1 + n] int32: the reference
    frame, its sources by ascending penalty -- ties by age in the buffer --, then -1; counts [M] int32) on the device,
    without synchronising.  The library refuses buffer_size > 64 and n_measurement_frames > 63."""
    import torch
    from . import _lib
    poses = _device_f64_poses(poses, device)
    if not isinstance(reference_indices, torch.Tensor) or not reference_indices.is_cuda:
        raise _lib.HipLibraryError("reference_indices must be a device tensor (no CPU fallback)")
    if reference_indices.dtype != torch.int32 or reference_indices.dim() != 1:
        raise TypeError(f"reference_indices must be [M] int32, got {tuple(reference_indices.shape)} {reference_indices.dtype}")
    refs = reference_indices.contiguous()
    n, M, N = int(n_measurement_frames), refs.shape[0], poses.shape[0]
    if n < 0:
        raise ValueError(f"n_measurement_frames = {n}")
    indices = torch.empty((M, 1 + n), dtype=torch.int32, device=poses.device)
    counts = torch.empty((M,), dtype=torch.int32, device=poses.device)
    inverses = pose_inverse(poses) if M else poses
    _lib.call("sr_tuple_walk_f64", poses.device, poses, inverses, N, refs, M, int(bool(both_directions)), int(buffer_size),
              int(buffer_size if acceptance_cap is None else acceptance_cap), float(keyframe_pose_distance),
              float(optimal_t), float(optimal_R), n, indices, counts)
    return indices, counts


def _device_tuples(scan, poses, reference_frames, n_measurement_frames, both_directions, device):
    import torch
    check_walk_poses(poses)
    device = torch.device(device)
    if device.type != "cuda":
        from . import _lib
        raise _lib.HipLibraryError(f"device {device}: the walk kernel runs on a GPU (device=None is the host path)")
    refs = torch.tensor(list(reference_frames), dtype=torch.int32).to(device)
    size = DVMVS_Config.test_keyframe_buffer_size * (2 if both_directions else 1)
    indices, _ = walk_tuples(torch.from_numpy(poses).to(device), refs, n_measurement_frames, both_directions, size,
                             device=device)
    samples = []
    for row in indices.cpu().tolist():      # the one device-to-host copy; -1 pads the rows
        sample = {"scan": scan, "indices": [v for v in row if v >= 0]}
        if _keep(sample, row[0]):
            samples.append(sample)
    return samples


def write_tuple_file(path, samples):
    """One line per tuple, `scan frame_id_0 frame_id_1 ...` with the reference frame first -- the file format the
    reference's datasets read (generate_test_tuples.py:1-8)."""
    with open(path, "w") as f:
        for s in samples:
            f.write(" ".join([str(s["scan"])] + [str(i) for i in s["indices"]]) + "\n")


def sort_sources_by_pose_penalty(cur_cam_T_world, src_world_T_cam):
    """Order of the source views as the reference's dataset feeds them to the model: ascending combined pose
    distance of cur_cam_T_src_cam (generic_mvs_dataset.py:643-659 with utils/geometry_utils.pose_distance :178-191).
    cur_cam_T_world [4,4], src_world_T_cam [K,4,4] (numpy or torch, fp32) -> list of K indices."""
    cur = np.asarray(cur_cam_T_world, dtype=np.float32)
    src = np.asarray(src_world_T_cam, dtype=np.float32)
    rel = cur[None] @ src                                        # cur_cam_T_src_cam, fp32 like the dataset's tensors
    tr = np.trace(rel[:, :3, :3], axis1=1, axis2=2)
    r_m = np.sqrt(2 * (1 - np.minimum(np.float32(3.0), tr) / 3))
    t_m = np.linalg.norm(rel[:, :3, 3], axis=1)
    return np.argsort(np.sqrt(t_m ** 2 + r_m ** 2), kind="stable").tolist()
