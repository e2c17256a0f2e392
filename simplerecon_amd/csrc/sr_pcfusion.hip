// sr_pcfusion.hip -- multi-view consistency fusion of depth maps into a point cloud, and voxel downsampling (the
// reference's pc_fusion.py: tools/torch_point_cloud_fusion.py:12-118, then open3d's voxel_down_sample).  gfx950 only.
//
// The rules are stated in include/simplerecon_hip.h, section "point-cloud fusion"; tests/pc_oracle.py implements them
// in fp64 numpy.
//   consistency : a thread per reference pixel walks every source frame in ascending order.  The per-frame constants
//                 are wave-uniform (scalar loads); the only vector memory traffic in the loop is one depth gather per
//                 (pixel, source).  Every workgroup walks the sources in the same order, so the source map being read
//                 is shared by all of them and stays in L2.  kUnroll projections are computed and their gathers issued
//                 before the first is consumed.  The running sum lives in registers: no atomics.
//   voxel keys  : fp64 floor-divide per point.
//   voxel mean  : a thread per occupied voxel sums its points in key-sorted (stable) order in fp64.
#include "sr_common.h"

// every fused multiply-add below is written out; nothing else may be contracted
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;   // sources in flight per thread
constexpr int kC = SR_PC_FRAME_FLOATS;

struct FuseParams {
  const float* depth;
  const float* consts;
  float* points;
  int* counts;
  int N, h, w, hw;
  int ref_begin;
  int blocks_per_frame;
  float z_thresh;
};

__global__ __launch_bounds__(kThreads) void sr_pc_consistency_kernel(FuseParams p) {
  const int fr = (int)blockIdx.x / p.blocks_per_frame;                  // frame within the chunk (uniform)
  const int pix = ((int)blockIdx.x - fr * p.blocks_per_frame) * kThreads + (int)threadIdx.x;
  const bool live = pix < p.hw;
  const int pc = live ? pix : p.hw - 1;   // idle lanes of the last block repeat the last pixel and store nothing
  const int r = p.ref_begin + fr;
  const int v = pc / p.w, u = pc - v * p.w;
  const float d = p.depth[(int64_t)r * p.hw + pc];
  const float fu = (float)u, fv = (float)v;
  const float* cr = p.consts + (int64_t)r * kC + 24;
  // step 1: X = d * (A (u, v, 1)) + a
  const float X0 = fmaf(d, fmaf(cr[0], fu, fmaf(cr[1], fv, cr[2])), cr[9]);
  const float X1 = fmaf(d, fmaf(cr[3], fu, fmaf(cr[4], fv, cr[5])), cr[10]);
  const float X2 = fmaf(d, fmaf(cr[6], fu, fmaf(cr[7], fv, cr[8])), cr[11]);
  float s0 = X0, s1 = X1, s2 = X2;
  int n = 0;
  const float wm1 = (float)(p.w - 1), hm1 = (float)(p.h - 1);

  for (int sb = 0; sb < p.N; sb += kUnroll) {
    // per source in flight: x, y, z and the sampled depth, which is NaN when the source is out of bounds (step 3) or
    // is the reference frame itself, so that step 5 fails for it
    float xs[kUnroll], ys[kUnroll], zq[kUnroll], zs[kUnroll];
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      const int s = sb + k < p.N ? sb + k : p.N - 1;   // past the end: a copy of the last source, never used
      const bool use = sb + k < p.N && s != r;          // wave-uniform
      const float* c = p.consts + (int64_t)s * kC;
      // step 2
      const float qx = fmaf(c[0], X0, fmaf(c[1], X1, fmaf(c[2], X2, c[3])));
      const float qy = fmaf(c[4], X0, fmaf(c[5], X1, fmaf(c[6], X2, c[7])));
      const float qz = fmaf(c[8], X0, fmaf(c[9], X1, fmaf(c[10], X2, c[11])));
      const float rz = __builtin_amdgcn_rcpf(qz);
      const float x = qx * rz, y = qy * rz;
      // step 3: a coordinate is in its closed interval iff clamping leaves it unchanged (NaN compares unequal)
      const bool in = use & (qz > 1e-4f) & (__builtin_amdgcn_fmed3f(x, 0.0f, wm1) == x) &
                      (__builtin_amdgcn_fmed3f(y, 0.0f, hm1) == y);
      // step 4: the nearest texel, clamped into the map whatever the coordinate, so the gather is always in bounds
      int ix = (int)__builtin_rintf(x), iy = (int)__builtin_rintf(y);
      ix = min(max(ix, 0), p.w - 1);
      iy = min(max(iy, 0), p.h - 1);
      const float* ds = p.depth + (int64_t)s * p.hw;
      const float z = ds[(uint32_t)(iy * p.w + ix)];
      xs[k] = x; ys[k] = y; zq[k] = qz;
      zs[k] = in ? z : __builtin_nanf("");
    }
#pragma unroll
    for (int k = 0; k < kUnroll; ++k) {
      const int s = sb + k < p.N ? sb + k : p.N - 1;
      const float* c = p.consts + (int64_t)s * kC + 12;
      // step 5
      const bool ok = __builtin_fabsf(zq[k] - zs[k]) < p.z_thresh;
      n += ok ? 1 : 0;
      // step 6: Y = z_s * (B (x, y, 1)) + b
      const float z = zs[k];
      const float Y0 = fmaf(z, fmaf(c[0], xs[k], fmaf(c[1], ys[k], c[2])), c[9]);
      const float Y1 = fmaf(z, fmaf(c[3], xs[k], fmaf(c[4], ys[k], c[5])), c[10]);
      const float Y2 = fmaf(z, fmaf(c[6], xs[k], fmaf(c[7], ys[k], c[8])), c[11]);
      // step 7
      const bool add = ok & !__builtin_isnan(Y0) & !__builtin_isnan(Y1) & !__builtin_isnan(Y2);
      s0 += add ? Y0 : 0.0f;
      s1 += add ? Y1 : 0.0f;
      s2 += add ? Y2 : 0.0f;
    }
  }
  if (!live) return;
  const float den = (float)(n + 1);
  float* out = p.points + (int64_t)fr * p.hw * 3;
  out[pix * 3 + 0] = s0 / den;
  out[pix * 3 + 1] = s1 / den;
  out[pix * 3 + 2] = s2 / den;
  p.counts[(int64_t)fr * p.hw + pix] = n;
}

constexpr int64_t kAxis = (int64_t)1 << 21;

__global__ __launch_bounds__(kThreads) void sr_pc_voxel_key_kernel(const float* __restrict__ pts, int64_t M, double mx,
                                                                   double my, double mz, double vs,
                                                                   int64_t* __restrict__ keys) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < M; i += (int64_t)gridDim.x * kThreads) {
    const double m[3] = {mx, my, mz};
    int64_t key = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double f = floor(((double)pts[i * 3 + a] - m[a]) / vs);
      const int64_t ia = f < 0.0 ? 0 : (f >= (double)(kAxis - 1) ? kAxis - 1 : (int64_t)f);   // NaN -> kAxis - 1
      key = key * kAxis + ia;
    }
    keys[i] = key;
  }
}

__global__ __launch_bounds__(kThreads) void sr_pc_voxel_mean_kernel(const float* __restrict__ pts,
                                                                    const uint8_t* __restrict__ cols, int64_t M,
                                                                    const int64_t* __restrict__ order,
                                                                    const int64_t* __restrict__ seg, int64_t S,
                                                                    float* __restrict__ out_pts,
                                                                    uint8_t* __restrict__ out_cols) {
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < S; v += (int64_t)gridDim.x * kThreads) {
    const int64_t b = seg[v], e = seg[v + 1];
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
    uint64_t c0 = 0, c1 = 0, c2 = 0;
    int64_t cnt = 0;
    for (int64_t j = b; j < e; ++j) {
      const int64_t i = order[j];
      if (i < 0 || i >= M) continue;   // not a permutation: skipped rather than read out of bounds
      a0 += (double)pts[i * 3 + 0];
      a1 += (double)pts[i * 3 + 1];
      a2 += (double)pts[i * 3 + 2];
      if (cols) {
        c0 += cols[i * 3 + 0];
        c1 += cols[i * 3 + 1];
        c2 += cols[i * 3 + 2];
      }
      ++cnt;
    }
    const double dc = (double)(cnt > 0 ? cnt : 1);
    out_pts[v * 3 + 0] = (float)(a0 / dc);
    out_pts[v * 3 + 1] = (float)(a1 / dc);
    out_pts[v * 3 + 2] = (float)(a2 / dc);
    if (cols && out_cols) {
      const uint64_t uc = (uint64_t)(cnt > 0 ? cnt : 1);
      out_cols[v * 3 + 0] = (uint8_t)((c0 + uc / 2) / uc);
      out_cols[v * 3 + 1] = (uint8_t)((c1 + uc / 2) / uc);
      out_cols[v * 3 + 2] = (uint8_t)((c2 + uc / 2) / uc);
    }
  }
}

unsigned grid_for(int64_t items) {
  const int64_t b = (items + kThreads - 1) / kThreads;
  return (unsigned)(b < 8192 ? (b > 0 ? b : 1) : 8192);
}

}  // namespace

extern "C" int sr_pc_consistency(const float* depth, const float* frame_consts, int N, int h, int w, int ref_begin,
                                 int ref_count, float z_thresh, float* points, int* counts, void* stream) {
  if (!depth || !frame_consts || !points || !counts) return SR_ERR_INVALID_ARGUMENT;
  if (N < 1 || h < 2 || w < 2) return SR_ERR_INVALID_ARGUMENT;
  if (ref_count < 1 || ref_begin < 0 || ref_begin > N - ref_count) return SR_ERR_INVALID_ARGUMENT;
  if (!(z_thresh > 0.0f) || !__builtin_isfinite(z_thresh)) return SR_ERR_INVALID_ARGUMENT;
  const int64_t hw = (int64_t)h * w;
  // per-frame offsets (pixel * 3 floats, in bytes) and the chunk's block count must fit int32
  if (hw * 3 * (int64_t)sizeof(float) > INT32_MAX) return SR_ERR_INVALID_ARGUMENT;
  if ((int64_t)ref_count * hw * 3 * (int64_t)sizeof(float) > INT32_MAX) return SR_ERR_INVALID_ARGUMENT;
  FuseParams P;
  P.depth = depth;
  P.consts = frame_consts;
  P.points = points;
  P.counts = counts;
  P.N = N; P.h = h; P.w = w; P.hw = (int)hw;
  P.ref_begin = ref_begin;
  P.blocks_per_frame = (int)((hw + kThreads - 1) / kThreads);
  P.z_thresh = z_thresh;
  const int64_t blocks = (int64_t)P.blocks_per_frame * ref_count;
  hipLaunchKernelGGL(sr_pc_consistency_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, P);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_pc_voxel_keys(const float* points, int64_t M, double min_x, double min_y, double min_z,
                                double voxel_size, int64_t* keys, void* stream) {
  if (M < 0 || (M > 0 && (!points || !keys))) return SR_ERR_INVALID_ARGUMENT;
  if (!(voxel_size > 0.0) || !__builtin_isfinite(voxel_size)) return SR_ERR_INVALID_ARGUMENT;
  if (!__builtin_isfinite(min_x) || !__builtin_isfinite(min_y) || !__builtin_isfinite(min_z))
    return SR_ERR_INVALID_ARGUMENT;
  if (M == 0) return SR_OK;
  hipLaunchKernelGGL(sr_pc_voxel_key_kernel, dim3(grid_for(M)), dim3(kThreads), 0, (hipStream_t)stream, points, M,
                     min_x, min_y, min_z, voxel_size, keys);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_pc_voxel_mean(const float* points, const uint8_t* colors, int64_t M, const int64_t* order,
                                const int64_t* seg_start, int64_t S, float* out_points, uint8_t* out_colors,
                                void* stream) {
  if (M < 0 || S < 0 || S > M) return SR_ERR_INVALID_ARGUMENT;
  if (S == 0) return SR_OK;
  if (!points || !order || !seg_start || !out_points || (colors && !out_colors)) return SR_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(sr_pc_voxel_mean_kernel, dim3(grid_for(S)), dim3(kThreads), 0, (hipStream_t)stream, points,
                     colors, M, order, seg_start, S, out_points, out_colors);
  return sr_hip_rc(hipGetLastError());
}
