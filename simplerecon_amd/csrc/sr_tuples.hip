// sr_tuples.hip -- the per-frame walks of the reference's offline and dense tuple modes
// (data_scripts/generate_test_tuples.py:65-157, 268-382 on tools/keyframe_buffer.py:245-381), one wave per reference frame.
//
// A walk offers the frames around its reference frame, one at a time, to a bounded FIFO of keyframes: a candidate is
// admitted when its DVMVS pose distance to EVERY buffered pose reaches the keyframe distance.  The buffer holds at most
// 64 poses, so lane l keeps ring slot l in registers (frame index + the top three rows of the pose), the admission test
// is one ballot, and the walks of a scan -- independent of each other -- run side by side.  Everything is fp64, every
// global write an ordinary store to an address no other lane writes: the result is a function of the inputs alone.
//
// Poses must be finite with a bottom row of exactly 0 0 0 1 (the caller checks): then rows 0..2 of inv(A) @ B need only
// rows 0..2 of both factors, whatever the inverse's own bottom row rounds to.
#include "sr_common.h"

#define SR_TUPLE_WAVES 4      // waves (= reference frames) per workgroup; they share nothing
#define SR_TUPLE_AHEAD 4      // candidates whose loads are in flight ahead of the one being tested

// General 4x4 inverse by cofactors (no rigid-motion shortcut: tracker poses are not exactly orthonormal and the
// reference inverts with np.linalg.inv).  One lane per pose.
__global__ __launch_bounds__(64) void sr_pose_inverse_f64_kernel(const double* __restrict__ poses, double* __restrict__ out,
                                                                 int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double* m = poses + 16 * (size_t)i;
  const double a00 = m[0], a01 = m[1], a02 = m[2], a03 = m[3], a10 = m[4], a11 = m[5], a12 = m[6], a13 = m[7];
  const double a20 = m[8], a21 = m[9], a22 = m[10], a23 = m[11], a30 = m[12], a31 = m[13], a32 = m[14], a33 = m[15];
  // 2x2 minors of the upper and of the lower pair of rows
  const double s0 = a00 * a11 - a10 * a01, s1 = a00 * a12 - a10 * a02, s2 = a00 * a13 - a10 * a03;
  const double s3 = a01 * a12 - a11 * a02, s4 = a01 * a13 - a11 * a03, s5 = a02 * a13 - a12 * a03;
  const double c5 = a22 * a33 - a32 * a23, c4 = a21 * a33 - a31 * a23, c3 = a21 * a32 - a31 * a22;
  const double c2 = a20 * a33 - a30 * a23, c1 = a20 * a32 - a30 * a22, c0 = a20 * a31 - a30 * a21;
  const double det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0;
  const double r = 1.0 / det;
  double* o = out + 16 * (size_t)i;
  o[0] = (a11 * c5 - a12 * c4 + a13 * c3) * r;
  o[1] = (-a01 * c5 + a02 * c4 - a03 * c3) * r;
  o[2] = (a31 * s5 - a32 * s4 + a33 * s3) * r;
  o[3] = (-a21 * s5 + a22 * s4 - a23 * s3) * r;
  o[4] = (-a10 * c5 + a12 * c2 - a13 * c1) * r;
  o[5] = (a00 * c5 - a02 * c2 + a03 * c1) * r;
  o[6] = (-a30 * s5 + a32 * s2 - a33 * s1) * r;
  o[7] = (a20 * s5 - a22 * s2 + a23 * s1) * r;
  o[8] = (a10 * c4 - a11 * c2 + a13 * c0) * r;
  o[9] = (-a00 * c4 + a01 * c2 - a03 * c0) * r;
  o[10] = (a30 * s4 - a31 * s2 + a33 * s0) * r;
  o[11] = (-a20 * s4 + a21 * s2 - a23 * s0) * r;
  o[12] = (-a10 * c3 + a11 * c1 - a12 * c0) * r;
  o[13] = (a00 * c3 - a01 * c1 + a02 * c0) * r;
  o[14] = (-a30 * s3 + a31 * s1 - a32 * s0) * r;
  o[15] = (a20 * s3 - a21 * s1 + a22 * s0) * r;
}

// value of lane `lane` (wave-uniform) in every lane
__device__ __forceinline__ double sr_lane_f64(double v, int lane) {
  const unsigned long long u = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)u, lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(u >> 32), lane);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}

// pose_distance (keyframe_buffer.py:54-70) of rel = A^-1 @ B from rows 0..2 of A^-1 (ia, wave-uniform) and of B (pb, this
// lane's): R = sqrt(2 (1 - min(3, tr) / 3)), t = |rel[:3,3]|.  Python's min(3.0, x) keeps 3.0 unless x < 3.0.
__device__ __forceinline__ void sr_pose_measures(const double (&ia)[12], const double (&pb)[12], double& r_measure,
                                                 double& t_measure) {
  const double tr = (ia[0] * pb[0] + ia[1] * pb[4] + ia[2] * pb[8]) + (ia[4] * pb[1] + ia[5] * pb[5] + ia[6] * pb[9]) +
                    (ia[8] * pb[2] + ia[9] * pb[6] + ia[10] * pb[10]);
  const double t0 = ia[0] * pb[3] + ia[1] * pb[7] + ia[2] * pb[11] + ia[3];
  const double t1 = ia[4] * pb[3] + ia[5] * pb[7] + ia[6] * pb[11] + ia[7];
  const double t2 = ia[8] * pb[3] + ia[9] * pb[7] + ia[10] * pb[11] + ia[11];
  const double trc = tr < 3.0 ? tr : 3.0;
  r_measure = sqrt(2.0 * (1.0 - trc / 3.0));
  t_measure = sqrt(t0 * t0 + t1 * t1 + t2 * t2);
}

struct SrTupleWalk {
  const double* poses;      // [N,16]
  const double* inverses;   // [N,16]
  const int* refs;          // [M] reference frame of each walk
  int* indices;             // [M, 1 + n_meas]
  int* counts;              // [M]
  int N, M, both, buffer_size, cap, n_meas;
  double kf_dist, opt_t, opt_r;
};

// Frame offered at turn t of the walk around frame r, or a value outside [0, N) for a turn that offers nothing.  Both
// directions: forward on even turns, backward on odd ones, an exhausted direction still takes its turn
// (generate_test_tuples.py:111-136).  Backward only: r-1, r-2, ... (:310-320).
__device__ __forceinline__ int sr_walk_candidate(int r, int t, int both) {
  if (!both) return r - 1 - t;
  return (t & 1) ? r - 1 - (t >> 1) : r + 1 + (t >> 1);
}
__device__ __forceinline__ bool sr_walk_over(int r, int t, int both, int N) {
  if (!both) return r - 1 - t < 0;
  return r + 1 + (t >> 1) >= N && r - 1 - (t >> 1) < 0;
}

__global__ __launch_bounds__(64 * SR_TUPLE_WAVES) void sr_tuple_walk_f64_kernel(SrTupleWalk p) {
  const int lane = threadIdx.x & 63;
  const int m = __builtin_amdgcn_readfirstlane(blockIdx.x * SR_TUPLE_WAVES + (threadIdx.x >> 6));
  if (m >= p.M) return;
  const int N = p.N, B = p.buffer_size, stride = 1 + p.n_meas;
  int* row = p.indices + (size_t)m * stride;
  const int r = __builtin_amdgcn_readfirstlane(p.refs[m]);
  if (r < 0 || r >= N) {   // not a frame of this scan: an empty row
    if (lane < stride) row[lane] = -1;
    if (lane == 0) p.counts[m] = 0;
    return;
  }

  // Lanes 0..11 fetch rows 0..2 of a candidate's inverse, lanes 12..23 those of its pose: one 8-byte load per lane and
  // candidate, handed round with readlane when the candidate's turn comes.  (The other lanes repeat element 0.)
  const double* fetch_base = lane < 12 ? p.inverses + lane : p.poses + (lane < 24 ? lane - 12 : 0);
  auto fetch = [&](int t) {
    int c = sr_walk_candidate(r, t, p.both);
    c = c < 0 ? 0 : (c >= N ? N - 1 : c);   // a turn that offers nothing loads an in-range dummy
    return fetch_base[16 * (size_t)c];
  };

  // ring slot `lane`: frame index and pose rows 0..2.  The walk is primed with the reference frame in slot 0.
  int idx = r;
  double pb[12];
  {
    const double own = fetch_base[16 * (size_t)r];
#pragma unroll
    for (int k = 0; k < 12; ++k) pb[k] = sr_lane_f64(own, 12 + k);
  }
  int len = 1, head = 0, added = 0;   // wave-uniform; while len < B the head stays 0, so slot l is occupied iff l < len

  double ahead[SR_TUPLE_AHEAD];
#pragma unroll
  for (int j = 0; j < SR_TUPLE_AHEAD; ++j) ahead[j] = fetch(j);

  bool done = false;
  for (int t0 = 0; !done; t0 += SR_TUPLE_AHEAD) {
#pragma unroll
    for (int j = 0; j < SR_TUPLE_AHEAD; ++j) {
      const int t = t0 + j;
      if (sr_walk_over(r, t, p.both, N)) { done = true; break; }
      const int c = sr_walk_candidate(r, t, p.both);
      const double cur = ahead[j];
      ahead[j] = fetch(t + SR_TUPLE_AHEAD);
      if (c < 0 || c >= N) continue;        // this direction is exhausted: the turn passes
      double ic[12];
#pragma unroll
      for (int k = 0; k < 12; ++k) ic[k] = sr_lane_f64(cur, k);
      double r_m, t_m;
      sr_pose_measures(ic, pb, r_m, t_m);   // pose_distance(candidate, buffered) = inv(candidate) @ buffered
      const double combined = sqrt(t_m * t_m + r_m * r_m);
      const bool too_close = lane < len && combined < p.kf_dist;
      if (__ballot(too_close) == 0ull) {
        // deque(maxlen=B).append: a full buffer loses its oldest entry, whichever frame that is by now
        const int tail = len < B ? len : head;
        const bool mine = lane == tail;
#pragma unroll
        for (int k = 0; k < 12; ++k) {
          const double v = sr_lane_f64(cur, 12 + k);
          pb[k] = mine ? v : pb[k];
        }
        idx = mine ? c : idx;
        if (len < B) ++len;
        else head = head + 1 == B ? 0 : head + 1;
        ++added;
      }
      if (added >= p.cap) { done = true; break; }
    }
  }

  // Source choice (get_best_measurement_frames_for_0index, keyframe_buffer.py:357-381): the oldest entry is dropped, the
  // next one is the reference pose of the penalties AND one of the scored entries; min(n, entries - 1) are taken.
  const int left = len - 1;
  int n = p.n_meas < left - 1 ? p.n_meas : left - 1;
  if (n < 0) n = 0;
  if (n > 0) {
    int pos = lane - head;                    // age order in the buffer, 0 = oldest
    if (pos < 0) pos += B;
    const bool scored = lane < len && pos >= 1;
    const int first = head + 1 >= B ? head + 1 - B : head + 1;
    const int ref_frame = __builtin_amdgcn_readlane(idx, first);
    double ir[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) ir[k] = p.inverses[16 * (size_t)ref_frame + k];
    double r_m, t_m;
    sr_pose_measures(ir, pb, r_m, t_m);       // pose_distance(reference, measurement)
    const double r_diff = fabs(r_m - p.opt_r), t_diff = t_m - p.opt_t;
    double penalty = r_diff * r_diff + (t_diff < 0.0 ? 5.0 : 1.0) * (fabs(t_diff) * fabs(t_diff));
    if (!(penalty == penalty)) penalty = __builtin_inf();   // a total order, so the ranks are a permutation
    // rank = scored entries ahead of this one in (penalty, buffer position) order
    int rank = 0;
    for (int j = 0; j < len; ++j) {
      const double pj = sr_lane_f64(penalty, j);
      int posj = j - head;
      if (posj < 0) posj += B;
      if (posj >= 1 && (pj < penalty || (pj == penalty && posj < pos))) ++rank;
    }
    if (scored && rank < n) row[1 + rank] = idx;
  }
  if (lane == 0) {
    row[0] = r;
    p.counts[m] = n;
  }
  if (lane >= n && lane < p.n_meas) row[1 + lane] = -1;
}

extern "C" int sr_pose_inverse_f64(const double* poses, double* inverses, int n, void* stream) {
  if (n < 0) return SR_ERR_INVALID_ARGUMENT;
  if (n == 0) return SR_OK;
  if (!poses || !inverses || ((uintptr_t)poses | (uintptr_t)inverses) % 8 != 0) return SR_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(sr_pose_inverse_f64_kernel, dim3((n + 63) / 64), dim3(64), 0, (hipStream_t)stream, poses, inverses, n);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_tuple_walk_f64(const double* poses, const double* inverses, int n_poses, const int32_t* reference_indices,
                                 int n_walks, int both_directions, int buffer_size, int acceptance_cap,
                                 double keyframe_pose_distance, double optimal_t, double optimal_r, int n_measurement_frames,
                                 int32_t* indices, int32_t* counts, void* stream) {
  if (n_poses < 0 || n_walks < 0 || buffer_size < 1 || n_measurement_frames < 0 || n_poses > (1 << 28))
    return SR_ERR_INVALID_ARGUMENT;
  if (buffer_size > 64 || n_measurement_frames > 63) return SR_ERR_UNSUPPORTED;
  if (n_walks == 0) return SR_OK;
  if (!reference_indices || !indices || !counts || (n_poses > 0 && (!poses || !inverses))) return SR_ERR_INVALID_ARGUMENT;
  if (((uintptr_t)poses | (uintptr_t)inverses) % 8 != 0 ||
      ((uintptr_t)reference_indices | (uintptr_t)indices | (uintptr_t)counts) % 4 != 0)
    return SR_ERR_INVALID_ARGUMENT;
  SrTupleWalk p;
  p.poses = poses; p.inverses = inverses; p.refs = reference_indices; p.indices = indices; p.counts = counts;
  p.N = n_poses; p.M = n_walks; p.both = both_directions != 0; p.buffer_size = buffer_size; p.cap = acceptance_cap;
  p.n_meas = n_measurement_frames; p.kf_dist = keyframe_pose_distance; p.opt_t = optimal_t; p.opt_r = optimal_r;
  hipLaunchKernelGGL(sr_tuple_walk_f64_kernel, dim3((n_walks + SR_TUPLE_WAVES - 1) / SR_TUPLE_WAVES),
                     dim3(64 * SR_TUPLE_WAVES), 0, (hipStream_t)stream, p);
  return sr_hip_rc(hipGetLastError());
}
