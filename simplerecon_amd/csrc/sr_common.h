// sr_common.h -- shared device/host helpers for libsimplerecon_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "simplerecon_hip.h"

// Per-(batch, view) geometry record written by sr_geom_kernel into the workspace:
//   [0,12)  rows 0..2 of P = K_src @ T_src_cur      (reference utils/geometry_utils.py:78-80)
//   [12,15) t = T_cur_src[:3,3]  (source camera centre in the reference frame; cost_volume.py:654-669)
//   [15]    pose_dist  [16] R_measure  [17] t_measure  (geometry_utils.py:178-191)
#define SR_GEOM_STRIDE 20

#define SR_WAVE 64

// value of a run-time switch (include/simplerecon_hip.h, SR_OPT_*): one relaxed atomic load; the environment is read once, at the
// first access in the process (sr_options.hip)
int sr_opt(int id);

// CU count of the CURRENT device, cached per device index (sr_options.hip); 256 when the runtime cannot be asked
int sr_device_cus();

// Allows `kernel` (the host-side function pointer) `bytes` of dynamic LDS on the CURRENT device
// (hipFuncAttributeMaxDynamicSharedMemorySize).  The largest size granted is remembered per (kernel, device), so the
// runtime is asked once and again only for a larger size; a refusal is not remembered.  Returns the runtime's error.
hipError_t sr_allow_lds(const void* kernel, size_t bytes);

// What the calling thread's last launcher call ran (sr_options.hip): the launch site notes the kernel family, the integers
// that selected the template arguments (a..f, in the kernel's order: see sr_last_launch) and the padded problem the kernel
// works through -- m x n x k multiplies, m = 0 where no such count is kept.  Plain thread-local stores; sr_last_launch turns
// them into the record's kernel name and executed FLOPs.  A launcher with several kernels notes its main one.
enum SrKernel { SR_K_NONE = 0, SR_K_CONV, SR_K_WINO, SR_K_WINO_SPLIT, SR_K_WINO4, SR_K_PW, SR_K_PW_TILED, SR_K_STEM, SR_K_C1S,
                SR_K_T16 };
struct SrLaunchNote { int kernel, a, b, c, d, e, f; int64_t m, n, k; };
void sr_note_launch(const SrLaunchNote& note);

// Second stages of the deterministic backward sums (sr_conv_bwd.hip), shared with their 16-bit forms (sr_conv16_wgrad.hip):
// d_weight[co][ci][tap] = the `per` partial [tap][64 co][64 ci] slabs of each (co, ci) block added in index order, and
// d_bias[c] = the [blocks][C] partial sums added in block order.  Each returns the launch's error code.
int sr_wgrad_reduce_launch(const float* part, float* d_weight, int Cout, int Cin, int taps, int ci_blocks, int per, int blocks,
                           hipStream_t stream);
int sr_bias_partial_reduce_launch(const float* partial, int blocks, int C, float* d_bias, hipStream_t stream);

static inline int sr_hip_rc(hipError_t e) { return e == hipSuccess ? SR_OK : SR_ERR_HIP_BASE + (int)e; }

static inline size_t sr_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct SrPlanes {
  const float* ptr;
  int64_t sb, sd, sy, sx;
};

struct SrVolumeOut {
  float* cv;
  int64_t sb, sd, sp;
  float* lowest;   // [B,h,w] or null
  uint8_t* mask;   // [B,h,w] or null
};

// ----------------------------------------------------------------------------------------
// Geometry shared by the dot-product and the MLP sweep.  Written op-by-op in the reference's
// order with FP contraction OFF so that pixel coordinates, z', masks and bilinear weights are
// bit-identical to the fp32 CPU oracle (discontinuous decisions cannot flip).
// ----------------------------------------------------------------------------------------
struct SrSample {
  float zp;            // z' = q_z + 1e-8                    (geometry_utils.py:84)
  float pix_x, pix_y;  // q_x * s, q_y * s                   (geometry_utils.py:85-87)
  float w_nw, w_ne, w_sw, w_se;  // bilinear weights, already zeroed for out-of-image taps
  int o_nw, o_ne, o_sw, o_se;    // texel indices (y*w + x), clamped in-image
  bool any_tap;                  // at least one of the four taps lies inside the image
};

typedef float sr_f2v __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));   // accumulator of a 32x32 fp32 MFMA

// Integer tap origin (floats, unclamped) and the four bilinear weights of the unnormalised sampling position (ix, iy)
// (grid_sample, bilinear, zeros padding, align_corners=False): weights of out-of-image taps are zero.
// any_tap: some tap is inside the image -- tap (xi, yj) is valid iff column xi and row yj both are, so this is
// (vx0 | vx1) & (vy0 | vy1), the validity tests themselves and not a guess from the weights (a valid tap may weigh 0).
__device__ __forceinline__ void sr_bilinear_taps(float ix, float iy, int h, int w, float& fx0, float& fy0, float& w_nw,
                                                 float& w_ne, float& w_sw, float& w_se, bool& any_tap) {
#pragma clang fp contract(off)
  const sr_f2v ixy = {ix, iy};
  fx0 = floorf(ix);
  fy0 = floorf(iy);
  const sr_f2v f0 = {fx0, fy0};
  const sr_f2v f1 = f0 + 1.0f;
  const float fx1 = f1.x, fy1 = f1.y;
  const float wm = (float)(w - 1), hm = (float)(h - 1);
  // (bitwise & on purpose: short-circuit && makes hipcc emit divergent branches that split the
  // scheduling region the callers want to interleave with MFMAs)
  const bool vx0 = (fx0 >= 0.0f) & (fx0 <= wm), vx1 = (fx1 >= 0.0f) & (fx1 <= wm);
  const bool vy0 = (fy0 >= 0.0f) & (fy0 <= hm), vy1 = (fy1 >= 0.0f) & (fy1 <= hm);
  const sr_f2v a1 = f1 - ixy, a0 = ixy - f0;            // (ax1, ay1), (ax0, ay0)
  const sr_f2v wtop = sr_f2v{a1.x, a0.x} * a1.y;        // (ax1*ay1, ax0*ay1)
  const sr_f2v wbot = sr_f2v{a1.x, a0.x} * a0.y;        // (ax1*ay0, ax0*ay0)
  w_nw = (vx0 & vy0) ? wtop.x : 0.0f;
  w_ne = (vx1 & vy0) ? wtop.y : 0.0f;
  w_sw = (vx0 & vy1) ? wbot.x : 0.0f;
  w_se = (vx1 & vy1) ? wbot.y : 0.0f;
  any_tap = (vx0 | vx1) & (vy0 | vy1);
}
__device__ __forceinline__ void sr_bilinear_taps(float ix, float iy, int h, int w, float& fx0, float& fy0, float& w_nw,
                                                 float& w_ne, float& w_sw, float& w_se) {
  bool any_tap;
  sr_bilinear_taps(ix, iy, h, w, fx0, fy0, w_nw, w_ne, w_sw, w_se, any_tap);
}

// Core of the projection: everything up to the bilinear weights, with the UNCLAMPED integer tap origin (fx0, fy0) as
// floats.  sr_project_sample (clamped global texel offsets) and the LDS-staged sweep (tile footprints) both build on it,
// so their geometry is the same instruction sequence.
// x / y components run as packed fp32 pairs (v_pk_mul_f32 / v_pk_add_f32: IEEE per component, FP contraction off, so
// every value is bit-identical to the scalar formulation) -- half the VALU instructions of the projection.
struct SrSampleXY {
  float zp, pix_x, pix_y;
  float ix, iy;                  // unnormalised sampling position (texel units; may be anything, incl. NaN)
  float fx0, fy0;                // its floor = the NW tap
  float w_nw, w_ne, w_sw, w_se;  // bilinear weights, already zeroed for out-of-image taps
  bool any_tap;                  // at least one tap inside the image (sr_bilinear_taps)
};

__device__ __forceinline__ void sr_project_sample_xy(const float* __restrict__ g /*geom record*/,
                                                     float X0, float X1, float X2, int h, int w,
                                                     float inv_w, float inv_h, SrSampleXY& s) {
#pragma clang fp contract(off)
  const float eps = 1e-8f;
  const sr_f2v q01 = sr_f2v{g[0], g[4]} * X0 + sr_f2v{g[1], g[5]} * X1 + sr_f2v{g[2], g[6]} * X2 + sr_f2v{g[3], g[7]};
  const float q2 = g[8] * X0 + g[9] * X1 + g[10] * X2 + g[11];
  s.zp = q2 + eps;
  const float sc = (fabsf(q2) > eps) ? 1.0f / s.zp : 1.0f;
  const sr_f2v pix = q01 * sc;
  s.pix_x = pix.x;
  s.pix_y = pix.y;
  // uv = 2*pix*(1/w,1/h) - 1 (cost_volume.py:199); grid_sample unnormalise, align_corners=False
  const sr_f2v uv = 2.0f * pix * sr_f2v{inv_w, inv_h} - 1.0f;
  const sr_f2v size = {(float)w, (float)h};
  const sr_f2v ixy = ((uv + 1.0f) * size - 1.0f) / 2.0f;
  s.ix = ixy.x;
  s.iy = ixy.y;
  sr_bilinear_taps(s.ix, s.iy, h, w, s.fx0, s.fy0, s.w_nw, s.w_ne, s.w_sw, s.w_se, s.any_tap);
}

__device__ __forceinline__ void sr_project_sample(const float* __restrict__ g /*geom record*/,
                                                  float X0, float X1, float X2, int h, int w,
                                                  float inv_w, float inv_h, SrSample& s) {
  SrSampleXY c;
  sr_project_sample_xy(g, X0, X1, X2, h, w, inv_w, inv_h, c);
  s.zp = c.zp; s.pix_x = c.pix_x; s.pix_y = c.pix_y;
  s.w_nw = c.w_nw; s.w_ne = c.w_ne; s.w_sw = c.w_sw; s.w_se = c.w_se;
  s.any_tap = c.any_tap;
  const float wm = (float)(w - 1), hm = (float)(h - 1);
  const float fx1 = c.fx0 + 1.0f, fy1 = c.fy0 + 1.0f;
  // clamp (NaN-safe: fmaxf(NaN, 0) = 0) so every tap address is in-image; weight 0 kills it
  const int x0 = (int)fminf(fmaxf(c.fx0, 0.0f), wm), x1 = (int)fminf(fmaxf(fx1, 0.0f), wm);
  const int y0 = (int)fminf(fmaxf(c.fy0, 0.0f), hm), y1 = (int)fminf(fmaxf(fy1, 0.0f), hm);
  s.o_nw = y0 * w + x0;
  s.o_ne = y0 * w + x1;
  s.o_sw = y1 * w + x0;
  s.o_se = y1 * w + x1;
}

// bounds test of get_mask (cost_volume.py:77-97)
__device__ __forceinline__ bool sr_in_bounds(const SrSample& s, int h, int w) {
  return (s.pix_x > 2.0f) & (s.pix_x < (float)(w - 2)) & (s.pix_y > 2.0f) & (s.pix_y < (float)(h - 2));
}

// Back-projected ray of pixel (x, y) through the 4x4 inverse intrinsics iK: r = iK[:3,:3] (x + 0.5, y + 0.5, 1)
// (geometry_utils.py:34-44); the point at plane depth d is d * r (geometry_utils.py:56-57).
__device__ __forceinline__ void sr_pixel_ray(const float* iK, int x, int y, float& r0, float& r1, float& r2) {
#pragma clang fp contract(off)
  const float px = (float)x + 0.5f, py = (float)y + 0.5f;
  r0 = iK[0] * px + iK[1] * py + iK[2];
  r1 = iK[4] * px + iK[5] * py + iK[6];
  r2 = iK[8] * px + iK[9] * py + iK[10];
}

// Activation code carried by the `leaky_slope` argument of the convolution entry points (simplerecon_hip.h): a value
// >= 0 is the LeakyReLU slope (0 = ReLU), SR_ACT_NONE (any value in (-1.5, 0)) the identity, SR_ACT_SILU x * sigmoid(x).
#ifdef __HIPCC__
// max / min as ONE instruction.  fmaxf() compiles to two: hipcc first canonicalises an operand it cannot prove quiet
// (v_max x, x, x) although in IEEE mode the instruction itself already returns a quiet result -- and it folds
// v_med3(a, b, inf) back into the same thing, so this is inline asm.  The compiler's hazard recogniser does not look
// inside inline asm: a (non-MFMA) VALU write needs 2 wait states before an MFMA reads the register (measured: wrong
// volumes in the W2-streaming MLP sweep without them), hence the `s_nop 1` in the _mfma form.  The plain form is for
// values that go to VALU arithmetic / stores.  For ordinary computed values (activations): NaN handling = v_max's.
__device__ __forceinline__ float sr_vmax(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float sr_vmin(float a, float b) {
  float r;
  asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float sr_vmax_mfma(float a, float b) {   // result may be an MFMA operand
  float r;
  asm("v_max_f32 %0, %1, %2\n\ts_nop 1" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ float sr_activate(float v, float slope) {
  if (slope >= 0.0f) return fmaxf(v, 0.0f) + slope * fminf(v, 0.0f);
  if (slope < -1.5f) return v / (1.0f + __expf(-v));
  return v;
}
// A wave-uniform float moved to a scalar register, so that a test on it is ONE s_cmp / s_cbranch instead of a vector
// compare + branch per value it guards.
__device__ __forceinline__ float sr_uniform(float x) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x)));
}
// sr_activate on a GROUP of values with the activation code tested once per group (r03: per value, the 32 outputs a
// Winograd epilogue thread owns cost 111 conditional branches around the SiLU code per region).  `slope` must be
// wave-uniform (pass it through sr_uniform).  LeakyReLU with 0 <= slope <= 1 is max(v, slope v) -- the same value as
// max(v,0) + slope min(v,0) for every finite v, in 1.5 instead of 3 instructions per value (v_pk_mul_f32 + v_max_f32).
template <int N>
__device__ __forceinline__ void sr_activate_group(float (&v)[N], float slope) {
  if (slope >= 0.0f) {
    if (slope <= 1.0f) {
#pragma unroll
      for (int i = 0; i < N; ++i) v[i] = sr_vmax(v[i], slope * v[i]);
    } else {
#pragma unroll
      for (int i = 0; i < N; ++i) v[i] = sr_vmax(v[i], 0.0f) + slope * sr_vmin(v[i], 0.0f);
    }
  } else if (slope < -1.5f) {
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = v[i] / (1.0f + __expf(-v[i]));
  }
}
#endif

// launch parameters of the dot-product sweeps (sr_dot_volume.hip, sr_dot_volume_lds.hip)
struct SrDotParams {
  const float* cur;       // [B,C,h,w]
  const float* src_nhwc;  // [B*K, h*w, C]
  const float* invK;      // [B,16]
  const float* geom;      // [B*K, SR_GEOM_STRIDE]
  SrPlanes planes;
  SrVolumeOut out;
  int B, K, h, w, D;
  float inv_w, inv_h;
};

// ---- stages shared by the L1-gather sweeps sr_dot_volume_kernel<C> and sr_dot_volume_kernel16q (sr_dot_volume.hip) ----
// What a lane of those kernels works on: a wavefront owns 64 consecutive pixels and the planes [j0, j1) of its plane group.
// Plane groups (grp of S, read by the kernel): waves of one workgroup (LDS argmax merge,
// sr_dot_store_lowest), or -- when there are too few pixel tiles to balance 256 CUs -- separate single-wave workgroups
// along grid z (lowest cost then comes from sr_argmax_planes).
// XCD-aware tile order: workgroup id % 8 selects the XCD (observed dispatch order; speed only, never correctness), so give
// each XCD a CONTIGUOUS band of pixel tiles -- its private L2 then holds one band (plus the disparity range) of every
// source map instead of all of them.  Bijective for any grid size.
struct SrDotLane {
  int lane, grp, S, b, N, tile;
  int pix, pc, y, x;   // this lane's pixel; pc = pix clamped into the image (what inactive lanes load from), (y, x) of pc
  bool active;         // pix < N
  int j0, j1;
};
__device__ __forceinline__ SrDotLane sr_dot_lane(const SrDotParams& p, int grp, int S) {
  SrDotLane l;
  l.lane = threadIdx.x & 63;
  l.grp = grp;
  l.S = S;
  l.b = blockIdx.y;
  l.N = p.h * p.w;
  l.tile = blockIdx.x;
  {
    const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, xcd = l.tile & 7, idx = l.tile >> 3;
    l.tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  }
  l.pix = l.tile * 64 + l.lane;
  l.active = l.pix < l.N;
  l.pc = l.active ? l.pix : l.N - 1;
  l.y = l.pc / p.w;
  l.x = l.pc - l.y * p.w;
  const int per = (p.D + l.S - 1) / l.S;
  l.j0 = l.grp * per;
  l.j1 = min(p.D, l.j0 + per);
  return l;
}
// running argmax over a lane's planes: first max wins; NaN = max (torch.argmax)
__device__ __forceinline__ void sr_argmax_step(float cost, float d, float& best, float& best_d, bool& have) {
  if (!have || cost > best || (cost != cost && best == best)) { best = cost; best_d = d; have = true; }
}
// lowest-cost depth of a pixel from its plane groups' running argmaxes; smem: [S][64] best cost, [S][64] best depth,
// [S][64] valid flag
__device__ __forceinline__ void sr_dot_store_lowest(const SrDotParams& p, const SrDotLane& l, float* smem, float best,
                                                    float best_d, bool have) {
  if (p.out.lowest) {
    if (gridDim.z > 1) {
      // merged by the caller (separate launch)
    } else if (l.S == 1) {
      if (l.active) p.out.lowest[(size_t)l.b * l.N + l.pix] = best_d;
    } else {
      float* s_best = smem;
      float* s_d = smem + l.S * 64;
      float* s_have = smem + 2 * l.S * 64;
      s_best[l.grp * 64 + l.lane] = best;
      s_d[l.grp * 64 + l.lane] = best_d;
      s_have[l.grp * 64 + l.lane] = have ? 1.0f : 0.0f;
      __syncthreads();
      if (l.grp == 0 && l.active) {
        float bb = best, bd = best_d;  // group 0 always owns plane 0
        for (int g = 1; g < l.S; ++g)
          if (s_have[g * 64 + l.lane] != 0.0f &&
              (s_best[g * 64 + l.lane] > bb || (s_best[g * 64 + l.lane] != s_best[g * 64 + l.lane] && bb == bb))) {
            bb = s_best[g * 64 + l.lane];
            bd = s_d[g * 64 + l.lane];
          }
        p.out.lowest[(size_t)l.b * l.N + l.pix] = bd;
      }
    }
  }
}

// workspace carving: [geom records | channels-last source features | per-pixel argmax keys of the LDS-staged sweep]
static inline float* sr_ws_geom(void* workspace) { return (float*)sr_align_up((size_t)workspace, 256); }
static inline float* sr_ws_src_nhwc(void* workspace, int B, int K) {
  return (float*)((char*)sr_ws_geom(workspace) + sr_align_up((size_t)B * K * SR_GEOM_STRIDE * sizeof(float), 256));
}

static inline size_t sr_ws_nhwc_bytes(int B, int K, int C, int h, int w) {
  return sr_align_up((size_t)B * K * h * w * C * sizeof(float), 256);
}
static inline unsigned long long* sr_ws_keys(void* workspace, int B, int K, int C, int h, int w) {
  return (unsigned long long*)((char*)sr_ws_src_nhwc(workspace, B, K) + sr_ws_nhwc_bytes(B, K, C, h, w));
}

// internal launchers shared between translation units
// LDS-staged 16-channel dot-product sweep (sr_dot_volume_lds.hip); SR_ERR_UNSUPPORTED when the shape is outside its
// range (the caller then takes the L1-gather kernels)
int sr_launch_dot_volume_lds(const SrDotParams& p, unsigned long long* keys, hipStream_t stream);
int sr_launch_geom(const float* K_src, const float* T_src_cur, const float* T_cur_src, float* geom,
                   int n, hipStream_t stream);
int sr_launch_argmax_planes(const float* cv, int64_t sb, int64_t sd, int64_t sp, SrPlanes planes, int B, int h, int w,
                            int D, float* lowest, hipStream_t stream);
// out = act(sum_k part[k * part_stride + ...] + bias + res): finish of a split-K convolution (partials dense
// channels-last [B, HW, Cout], Cout % 4 == 0, 16-byte aligned operands); defined in sr_wino.hip
int sr_launch_splitk_reduce(const float* part, int ksplit, int64_t part_stride, const float* bias, const float* res,
                            int64_t res_sb, int res_sp, float* out, int64_t out_sb, int out_sp, int B, int HW, int Cout,
                            float slope, hipStream_t stream);
// [images, npix, C] -> [images, C, npix] (C % 4 == 0); defined in sr_dot_volume_bwd.hip
int sr_launch_unpack_nhwc(const float* src_nhwc, float* dst_nchw, int images, int C, int npix, hipStream_t stream);
int sr_launch_pack_nhwc(const float* src_nchw, float* dst_nhwc, int images, int C, int npix,
                        hipStream_t stream);
