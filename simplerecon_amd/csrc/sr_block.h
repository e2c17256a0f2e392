// sr_block.h -- building blocks shared by the scene-side kernels (losses, metrics, mesh metrics, dense and sparse mesh
// extraction).  Device only; include after sr_common.h.  One definition per rule: several callers pin their results bit
// for bit, so a change here changes all of them together.
#pragma once
#include "sr_common.h"

// Sum of v over the wave, in every lane (butterfly: the same order of additions on every run).
template <typename T>
__device__ __forceinline__ T sr_wave_sum(T v) {
#pragma unroll
  for (int o = SR_WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// F.interpolate(mode="nearest") source index along one axis: ATen's identity and exact-2x cases, else
// min(floor(dst * (in / out)), in - 1) with the scale and the product in fp32 (nearest_idx).  A divide, a multiply and
// a floor, in that order: there is no multiply-add to contract, whatever the including file's fp contract setting.
__device__ __forceinline__ int sr_nearest_src(int dst, int in, int out) {
  if (in == out) return dst;
  if (out == 2 * in) return dst >> 1;
  const float scale = (float)in / (float)out;
  const int s = (int)floorf((float)dst * scale);
  return s < in - 1 ? s : in - 1;
}

// Exclusive scan of N int counters over a workgroup of THREADS threads (Hillis-Steele in LDS), and the workgroup totals.
// Every thread of the workgroup calls it.  The trailing barrier frees the LDS array for the next call.
template <int N, int THREADS>
__device__ __forceinline__ void sr_block_scan(const int (&v)[N], int (&excl)[N], int (&total)[N]) {
  __shared__ int s[THREADS][N];
  const int t = threadIdx.x;
#pragma unroll
  for (int c = 0; c < N; ++c) s[t][c] = v[c];
  __syncthreads();
#pragma unroll 1
  for (int d = 1; d < THREADS; d <<= 1) {
    int o[N] = {};
    if (t >= d) {
#pragma unroll
      for (int c = 0; c < N; ++c) o[c] = s[t - d][c];
    }
    __syncthreads();
    if (t >= d) {
#pragma unroll
      for (int c = 0; c < N; ++c) s[t][c] += o[c];
    }
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < N; ++c) {
    excl[c] = s[t][c] - v[c];
    total[c] = s[THREADS - 1][c];
  }
  __syncthreads();
}

// Index of `key` in the ascending array keys[lo, hi), or -1.
__device__ __forceinline__ int64_t sr_find_sorted(const int64_t* keys, int64_t lo, int64_t hi, int64_t key) {
  const int64_t end = hi;
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return (lo < end && keys[lo] == key) ? lo : -1;
}
