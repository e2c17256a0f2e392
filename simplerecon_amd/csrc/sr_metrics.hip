// sr_metrics.hip -- the reference's depth metrics (utils/metrics_utils.py compute_depth_metrics_batched /
// compute_depth_metrics, scored as test.py:203-455 and experiment_modules/depth_model.py:573-596 do).  gfx950 only.
//
// The rules are stated in include/simplerecon_hip.h, section "depth metrics"; tests/metrics_oracle.py restates them in
// numpy.  Two launches per call:
//   tile pass : a block per (frame, tile of kTilePix gt pixels).  Each thread reads 4 consecutive gt pixels per step
//               (one float4 when the frame base allows it), gathers the prediction in place (identity or nearest:
//               the source pixel F.interpolate(mode="nearest") picks; the upsampled map is never written), computes
//               the fp32 per-pixel terms in the reference's order and accumulates them in fp64.  The block writes one
//               record of kFields doubles: the valid count, (sum, count) of the non-NaN terms of the five error
//               metrics, and the five threshold counts.
//   finalize  : one workgroup.  A wave per frame reduces that frame's records in a fixed order, writes its 12 metrics
//               and its valid count; the per-frame totals are then summed in frame order for the pooled metrics.
// The record layout of a frame depends only on (H, W, h, w), so a frame's metrics have the same bits whatever batch it
// is scored in.  No float atomics, no host synchronisation.
#include <math.h>

#include "sr_common.h"
#include "sr_block.h"

#pragma clang fp contract(off)

namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / SR_WAVE;
constexpr int kVec = 4;                       // gt pixels per thread and step
constexpr int kSteps = 4;                     // steps per thread
constexpr int kTilePix = kT * kVec * kSteps;  // 4096 gt pixels per record
constexpr int kFields = 16;                   // n, (sum, count) x 5 error terms, 5 threshold counts
constexpr int kMaxPix = SR_METRICS_MAX_PIXELS;   // H*W bound: counts are exact in fp32 and int32

// The thresholds of the a-metrics, compared in fp32: 1.05f, 1.1f, 1.25f, 1.25^2, 1.25^3.
__constant__ float kThresh[5] = {1.05f, 1.1f, 1.25f, 1.5625f, 1.953125f};

struct MetricParams {
  const float* gt;        // [B,H,W]
  const float* pred;      // [B,h,w]
  const uint8_t* mask;    // [B,H,W] or null: valid = gt > min_depth
  float min_depth;
  int H, W, h, w;
  int nearest;            // 0: identity (h == H, w == W)
  int vec_gt, vec_pred, vec_mask;   // 16-byte (mask: 4-byte) aligned frames: vector loads (same arithmetic either way)
  int tiles;              // records per frame
  double* records;        // [B, tiles, kFields]
};

__device__ __forceinline__ int gather_index(const MetricParams& p, int pix) {
  if (!p.nearest) return pix;
  const int y = pix / p.W, x = pix - y * p.W;
  return sr_nearest_src(y, p.h, p.H) * p.w + sr_nearest_src(x, p.w, p.W);
}

// One valid pixel's contribution, in the reference's operation order (fp32 terms, fp64 sums).
__device__ __forceinline__ void accumulate(float gt, float pr, double (&acc)[kFields]) {
  acc[0] += 1.0;
  const float d = gt - pr;
  const float ad = __builtin_fabsf(d);
  const float sq = d * d;
  const float lg = logf(gt) - logf(pr);
  const float terms[5] = {ad, ad / gt, sq / gt, sq, lg * lg};
#pragma unroll
  for (int m = 0; m < 5; ++m) {
    if (!__builtin_isnan(terms[m])) {
      acc[1 + 2 * m] += (double)terms[m];
      acc[2 + 2 * m] += 1.0;
    }
  }
  // torch.max(gt / pred, pred / gt): NaN if either is; a NaN ratio fails every threshold, and max(r1, r2) < t is
  // r1 < t && r2 < t for non-NaN ratios
  const float r1 = gt / pr, r2 = pr / gt;
#pragma unroll
  for (int k = 0; k < 5; ++k)
    if (r1 < kThresh[k] && r2 < kThresh[k]) acc[11 + k] += 1.0;
}

__global__ __launch_bounds__(kT) void sr_metrics_tile_kernel(MetricParams p) {
  const int tile = blockIdx.x, b = blockIdx.y;
  const int hw = p.H * p.W;
  const float* gt = p.gt + (int64_t)b * hw;
  const float* pred = p.pred + (int64_t)b * p.h * p.w;
  const uint8_t* mask = p.mask ? p.mask + (int64_t)b * hw : nullptr;
  double acc[kFields];
#pragma unroll
  for (int f = 0; f < kFields; ++f) acc[f] = 0.0;

  for (int s = 0; s < kSteps; ++s) {
    const int p0 = tile * kTilePix + (s * kT + (int)threadIdx.x) * kVec;
    if (p0 >= hw) break;
    float g[kVec], q[kVec];
    bool v[kVec];
    if (p.vec_gt) {   // hw % 4 == 0: all four pixels exist
      const float4 t = *reinterpret_cast<const float4*>(gt + p0);
      g[0] = t.x; g[1] = t.y; g[2] = t.z; g[3] = t.w;
    } else {
#pragma unroll
      for (int j = 0; j < kVec; ++j) g[j] = p0 + j < hw ? gt[p0 + j] : 0.0f;
    }
    if (mask) {
      if (p.vec_mask) {
        const uint32_t m = *reinterpret_cast<const uint32_t*>(mask + p0);
#pragma unroll
        for (int j = 0; j < kVec; ++j) v[j] = (m >> (8 * j)) & 0xffu;
      } else {
#pragma unroll
        for (int j = 0; j < kVec; ++j) v[j] = p0 + j < hw && mask[p0 + j] != 0;
      }
    } else {
#pragma unroll
      for (int j = 0; j < kVec; ++j) v[j] = p0 + j < hw && g[j] > p.min_depth;
    }
    if (p.vec_pred) {   // identity resampling with an aligned prediction
      const float4 t = *reinterpret_cast<const float4*>(pred + p0);
      q[0] = t.x; q[1] = t.y; q[2] = t.z; q[3] = t.w;
    } else {
#pragma unroll
      for (int j = 0; j < kVec; ++j) q[j] = v[j] ? pred[gather_index(p, p0 + j)] : 0.0f;
    }
#pragma unroll
    for (int j = 0; j < kVec; ++j)
      if (v[j]) accumulate(g[j], q[j], acc);
  }

  __shared__ double red[kWaves][kFields];
  const int lane = threadIdx.x & (SR_WAVE - 1), wv = threadIdx.x / SR_WAVE;
#pragma unroll
  for (int f = 0; f < kFields; ++f) {
    const double t = sr_wave_sum(acc[f]);
    if (lane == 0) red[wv][f] = t;
  }
  __syncthreads();
  if ((int)threadIdx.x < kFields) {
    double t = red[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) t += red[k][threadIdx.x];
    p.records[((int64_t)b * p.tiles + tile) * kFields + threadIdx.x] = t;
  }
}

struct FinalParams {
  const double* records;   // [B, tiles, kFields]
  double* totals;          // [B, kFields] (scratch)
  int B, tiles, mult_a;
  float* out_frame;        // [B,12]
  int32_t* out_count;      // [B]
  float* out_pooled;       // [12] or null
};

// The 12 metrics in the reference's key order from one set of totals.  pooled: plain means (a NaN term makes the metric
// NaN); else nanmean per error metric.  An empty mean is 0 / 0 = NaN.
__device__ void write_metrics(const double* t, bool pooled, int mult_a, float* o) {
  const double n = t[0];
  double mean[5];
#pragma unroll
  for (int m = 0; m < 5; ++m) {
    const double c = t[2 + 2 * m];
    mean[m] = (pooled && c != n) ? __builtin_nan("") : t[1 + 2 * m] / c;
  }
  o[0] = (float)mean[0];         // abs_diff
  o[1] = (float)mean[1];         // abs_rel
  o[2] = (float)mean[2];         // sq_rel
  o[3] = (float)sqrt(mean[3]);   // rmse
  o[4] = (float)sqrt(mean[4]);   // rmse_log
  float a[5];
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    a[k] = (float)(t[11 + k] / n);
    if (mult_a) a[k] = a[k] * 100.0f;
  }
  o[5] = a[0];    // a5
  o[6] = a[1];    // a10
  o[7] = a[2];    // a25
  o[8] = a[1];    // a0 = a10
  o[9] = a[2];    // a1 = a25
  o[10] = a[3];   // a2
  o[11] = a[4];   // a3
}

__global__ __launch_bounds__(kT) void sr_metrics_finalize_kernel(FinalParams p) {
  const int lane = threadIdx.x & (SR_WAVE - 1), wv = threadIdx.x / SR_WAVE;
  constexpr int kSub = SR_WAVE / kFields;   // 4 record streams per field
  const int f = lane % kFields, sub = lane / kFields;
  for (int b = wv; b < p.B; b += kWaves) {
    const double* r = p.records + (int64_t)b * p.tiles * kFields;
    double s = 0.0;
    for (int t = sub; t < p.tiles; t += kSub) s += r[(int64_t)t * kFields + f];
    s += __shfl_xor(s, kFields);       // every lane now holds the total of its field
    s += __shfl_xor(s, 2 * kFields);
    if (lane < kFields) p.totals[(int64_t)b * kFields + f] = s;
    double t[kFields];
#pragma unroll
    for (int k = 0; k < kFields; ++k) t[k] = __shfl(s, k);
    if (lane == 0) {
      write_metrics(t, false, p.mult_a, p.out_frame + (int64_t)b * 12);
      p.out_count[b] = (int32_t)t[0];
    }
  }
  if (!p.out_pooled) return;
  __syncthreads();
  __shared__ double pooled[kFields];
  if ((int)threadIdx.x < kFields) {
    double s = 0.0;
    for (int b = 0; b < p.B; ++b) s += p.totals[(int64_t)b * kFields + threadIdx.x];
    pooled[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) write_metrics(pooled, true, p.mult_a, p.out_pooled);
}

__global__ __launch_bounds__(kT) void sr_metrics_gather_kernel(MetricParams p, float* out) {
  const int b = blockIdx.y;
  const int pix = blockIdx.x * kT + threadIdx.x;
  if (pix >= p.H * p.W) return;
  out[(int64_t)b * p.H * p.W + pix] = p.pred[(int64_t)b * p.h * p.w + gather_index(p, pix)];
}

int tiles_for(int H, int W) { return (int)(((int64_t)H * W + kTilePix - 1) / kTilePix); }

bool shape_ok(int B, int H, int W, int h, int w, int resample) {
  if (B < 1 || B > 65535 || H < 1 || W < 1 || h < 1 || w < 1) return false;
  if ((int64_t)H * W > kMaxPix || (int64_t)h * w > kMaxPix) return false;
  if (resample == SR_RESAMPLE_IDENTITY) return h == H && w == W;
  return resample == SR_RESAMPLE_NEAREST;
}

bool aligned(const void* ptr, size_t a) { return ((uintptr_t)ptr % a) == 0; }

}  // namespace

// ====================================================================================================================
extern "C" size_t sr_depth_metrics_workspace_bytes(int B, int H, int W) {
  if (B < 1 || B > 65535 || H < 1 || W < 1 || (int64_t)H * W > kMaxPix) return 0;
  return ((size_t)B * tiles_for(H, W) + (size_t)B) * kFields * sizeof(double);
}

extern "C" int sr_depth_metrics(const float* gt, const float* pred, const uint8_t* mask, float min_depth, int B, int H,
                                int W, int h, int w, int resample, int mult_a, float* out_frame, int32_t* out_count,
                                float* out_pooled, void* workspace, size_t workspace_bytes, void* stream) {
  if (!gt || !pred || !out_frame || !out_count || !workspace) return SR_ERR_INVALID_ARGUMENT;
  if (!shape_ok(B, H, W, h, w, resample)) return SR_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < sr_depth_metrics_workspace_bytes(B, H, W)) return SR_ERR_WORKSPACE_TOO_SMALL;
  if (!aligned(workspace, sizeof(double))) return SR_ERR_INVALID_ARGUMENT;
  const int64_t hw = (int64_t)H * W;
  MetricParams P{};
  P.gt = gt; P.pred = pred; P.mask = mask; P.min_depth = min_depth;
  P.H = H; P.W = W; P.h = h; P.w = w;
  P.nearest = resample == SR_RESAMPLE_NEAREST && !(h == H && w == W);
  P.vec_gt = hw % 4 == 0 && aligned(gt, 16);
  P.vec_pred = !P.nearest && hw % 4 == 0 && aligned(pred, 16);
  P.vec_mask = mask && hw % 4 == 0 && aligned(mask, 4);
  P.tiles = tiles_for(H, W);
  P.records = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sr_metrics_tile_kernel, dim3(P.tiles, B), dim3(kT), 0, st, P);
  int rc = sr_hip_rc(hipGetLastError());
  if (rc) return rc;
  FinalParams F{};
  F.records = P.records;
  F.totals = P.records + (size_t)B * P.tiles * kFields;
  F.B = B; F.tiles = P.tiles; F.mult_a = mult_a ? 1 : 0;
  F.out_frame = out_frame; F.out_count = out_count; F.out_pooled = out_pooled;
  hipLaunchKernelGGL(sr_metrics_finalize_kernel, dim3(1), dim3(kT), 0, st, F);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_depth_metrics_gather(const float* pred, int B, int H, int W, int h, int w, int resample, float* out,
                                       void* stream) {
  if (!pred || !out || !shape_ok(B, H, W, h, w, resample)) return SR_ERR_INVALID_ARGUMENT;
  MetricParams P{};
  P.pred = pred; P.H = H; P.W = W; P.h = h; P.w = w;
  P.nearest = resample == SR_RESAMPLE_NEAREST && !(h == H && w == W);
  const dim3 grid((unsigned)(((int64_t)H * W + kT - 1) / kT), B);
  hipLaunchKernelGGL(sr_metrics_gather_kernel, grid, dim3(kT), 0, (hipStream_t)stream, P, out);
  return sr_hip_rc(hipGetLastError());
}
