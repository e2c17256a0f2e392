// sr_mlp_volume.hip -- fused plane sweep of the metadata-MLP feature volume for gfx950.
//
// Replaces FeatureVolumeManager.build_cost_volume / FastFeatureVolumeManager of the reference
// (modules/cost_volume.py:451-736, 967-1164): per depth plane ~40 ATen launches, a 202-channel
// concat tensor and two [B*N,128] hidden tensors (or, in the "fast" variant, 7.9 GB of them at
// batch 8).  Here a wavefront owns 64 points (64 pixels of one depth plane: an 8x8, 4x16 or 2x32 tile, or 64 consecutive
// pixels of the flattened map -- sr_mlp_lane_pixel):
//   * VALU part: homography, 4-tap bilinear gather of the channels-last source features,
//     dot / mask / depth / rays / ray angle -- each lane builds the MLP input vector of ITS point
//     in registers, never in memory;
//   * MFMA part (fp32 in, fp32 accumulate, v_mfma_f32_32x32x2_f32): H1^T = W1 . X^T and
//     H2^T = W2 . H1^T as two 32-point column groups.  One v_permlane32_swap per k-step turns two
//     per-lane feature registers into the B operands of both groups; the layer-1 accumulators ARE
//     the layer-2 B operands (the k order of W2 is permuted to the MFMA C layout on the host side),
//     so activations never touch LDS or HBM.  Layer 3 (128 -> 1) is a per-lane dot + one swap.
//   * W1 (packed in k-step order) lives in LDS for the whole persistent block; W2 streams from
//     L2 with a register prefetch (both do not fit the 160 KB LDS in fp32).
#include <stdlib.h>
#include <string.h>

#include "sr_buffer.h"
#include "sr_view.h"

#define SR_HID 128          // hidden width of the matching MLP (reference cost_volume.py:402)
// Layer-1 inputs are split into a depth-VARIANT part (per view: 16 warped channels, mask, z', ray angle,
// source ray(3), dot and one spare slot that carries the plane depth d for view 0: sr_mlp_var_col) and a depth-INVARIANT
// part (reference features 16, reference ray 3, the constant 1 that carries the bias, 3 pose measures per
// view).  The invariant part is multiplied ONCE per (64-pixel tile, chunk of planes) and re-used as the
// accumulator initialiser of every plane of the chunk (-17 % layer-1 MFMA work).
#define SR_VIEW_SLOTS 24
#define SR_INV_FIXED 20     // cur(16), cur_ray(3), one
#define SR_PLANE_CHUNK 8    // planes per work unit

static inline int sr_mlp_steps_var(int K) { return (SR_VIEW_SLOTS / 2) * K; }
static inline int sr_mlp_steps_inv(int K) { return (SR_INV_FIXED + 3 * K + 1) / 2; }
static inline int sr_mlp_steps1(int K) { return sr_mlp_steps_var(K) + sr_mlp_steps_inv(K); }
#define SR_MLP_STEPS2 65    // 64 hidden pairs + one bias step

// packed parameter block (floats): [W1p: steps1*256 (variant steps first)][W2p: 65*256][w3tab: 128][b3: 1][pad]
static inline size_t sr_mlp_packed_floats(int K) { return (size_t)(sr_mlp_steps1(K) + SR_MLP_STEPS2) * 256 + 128 + 4; }

// ------------------------------------------------------------------ weight packing ----
// The one map from a layer-1 input slot of the sweep to its column of W1 [hidden, Cin] (reference channel offsets:
// cost_volume.py:709-723); both packers below and nothing else place W1 columns.  -1: no column (zero), -2: the bias.
// Slots of a view: 0..15 warped channels | 16 mask, 17 z' | 18 ray angle, 19 ray_0 | 20 ray_1, 21 ray_2 | 22 dot * mask,
// 23 spare (the plane depth d for view 0, nothing for k > 0).  One pair = one k-step (8..11), and the pair (22, 23) comes
// last: both are exact zeros for a dead view k > 0, so that view ends after step 10 (SR_VIEW_BODY).
#define SR_MLP_COLUMN_OFFSETS(K, C)                                                                    \
  const int o_cur = (K) * (C), o_mask = o_cur + (C), o_z = o_mask + (K), o_d = o_z + (K), o_dot = o_d + 1; \
  const int o_ang = o_dot + (K), o_cray = o_ang + (K), o_sray = o_cray + 3, o_pd = o_sray + 3 * (K);  \
  const int o_rm = o_pd + (K), o_tm = o_rm + (K);
__device__ __forceinline__ int sr_mlp_var_col(int K, int C, int k, int s) {   // slot s of view k (depth-variant part)
  SR_MLP_COLUMN_OFFSETS(K, C)
  (void)o_cur; (void)o_cray; (void)o_pd; (void)o_rm; (void)o_tm;
  if (s < 16) return k * C + s;
  if (s == 16) return o_mask + k;
  if (s == 17) return o_z + k;
  if (s == 18) return o_ang + k;
  if (s < 22) return o_sray + 3 * k + (s - 19);
  if (s == 22) return o_dot + k;
  return (k == 0) ? o_d : -1;
}
__device__ __forceinline__ int sr_mlp_inv_col(int K, int C, int u) {          // slot u of the depth-invariant part
  SR_MLP_COLUMN_OFFSETS(K, C)
  (void)o_mask; (void)o_z; (void)o_d; (void)o_dot; (void)o_ang; (void)o_sray;
  if (u < 16) return o_cur + u;
  if (u < 19) return o_cray + (u - 16);
  if (u == 19) return -2;
  if (u >= SR_INV_FIXED + 3 * K) return -1;
  const int k = (u - SR_INV_FIXED) / 3, i = (u - SR_INV_FIXED) - 3 * k;
  return (i == 0 ? o_pd : (i == 1 ? o_rm : o_tm)) + k;
}

// W?p[t][lane][mt] = W[row = 32*mt + (lane&31)][column of k-slot (t, half = lane>>5)]
__global__ void sr_mlp_pack_kernel(const float* __restrict__ W1, const float* __restrict__ b1,
                                   const float* __restrict__ W2, const float* __restrict__ b2,
                                   const float* __restrict__ W3, const float* __restrict__ b3,
                                   float* __restrict__ packed, int K, int C) {
  const int steps_var = (SR_VIEW_SLOTS / 2) * K;
  const int steps1 = steps_var + (SR_INV_FIXED + 3 * K + 1) / 2;
  const int Cin = C * (K + 1) + 10 * K + 4;
  const int total = (steps1 + SR_MLP_STEPS2) * 256 + 128 + 1;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    float v = 0.0f;
    if (e < steps1 * 256) {
      const int t = e >> 8, lane = (e >> 2) & 63, mt = e & 3;
      const int row = 32 * mt + (lane & 31);
      int col;
      if (t < steps_var) {
        const int slot = 2 * t + (lane >> 5);
        const int k = slot / SR_VIEW_SLOTS;
        col = sr_mlp_var_col(K, C, k, slot - k * SR_VIEW_SLOTS);
      } else {
        col = sr_mlp_inv_col(K, C, 2 * (t - steps_var) + (lane >> 5));
      }
      v = (col >= 0) ? W1[(size_t)row * Cin + col] : (col == -2 ? b1[row] : 0.0f);
    } else if (e < (steps1 + SR_MLP_STEPS2) * 256) {
      const int e2 = e - steps1 * 256;
      const int t = e2 >> 8, lane = (e2 >> 2) & 63, mt = e2 & 3;
      const int row = 32 * mt + (lane & 31);
      if (t < 64) {
        // k-step t = (m, r): hidden feature held by this half in accumulator register r of tile m
        const int m = t >> 4, r = t & 15;
        const int f = 32 * m + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        v = W2[(size_t)row * SR_HID + f];
      } else {
        v = (lane < 32) ? b2[row] : 0.0f;  // bias step: B operand is 1 in half 0
      }
    } else if (e < (steps1 + SR_MLP_STEPS2) * 256 + 128) {
      // w3tab[half][mt][r] = W3[feature of accumulator register r of tile mt in that half]
      const int i = e - (steps1 + SR_MLP_STEPS2) * 256;
      const int half = i >> 6, mt = (i >> 4) & 3, r = i & 15;
      v = W3[32 * mt + (r & 3) + 8 * (r >> 2) + 4 * half];
    } else {
      v = b3[0];
    }
    packed[e] = v;
  }
}

// ------------------------------------------------------------------ the sweep ---------

struct SrMlpParams {
  const float* cur;       // [B,16,h,w], or [B, h*w, 16] when cur_nhwc
  const float* src_nhwc;  // [B*K, h*w, 16]
  const float* invK;      // [B,16]
  const float* geom;      // [B*K, SR_GEOM_STRIDE]
  const float* packed;    // sr_mlp_pack_kernel output
  SrPlanes planes;
  SrVolumeOut out;
  int B, K, h, w, D;
  int tiles;              // 64-pixel tiles per image: tiles_x * ceil(h / th), or ceil(h*w / 64) for the flattened strip
  int tiles_x;            // th x tw tiles per tile row, ceil(w / tw); 0: the flattened strip (sr_mlp_lane_pixel)
  int th_log2, tw_log2;   // th * tw = 64
  int chunk, chunks;      // planes per work unit, ceil(D / chunk)
  int cur_nhwc;           // cur is channels-last like src (sr_mlp_volume_fwd_nhwc): a lane's 16 channels are one 64-byte run
  int vec_store;          // channels-last volume (plane stride 1): a lane keeps the costs of its unit's planes and
                          // stores them as 16-byte pieces at the end of the unit (instead of one 4-byte store per plane
                          // into 64 different 256-byte rows: r02 PMC counted 6.7x the volume's bytes in WRITE_SIZE)
  float inv_w, inv_h, slope;
};

// Which pixel a lane of the wave that owns `tile` works on.  Whether a view is dead for a wave (below) is a spatial
// property -- the live region is the source image shifted along the epipolar line -- so a compact th x tw tile (th * tw =
// 64, tiles row-major over (ty, tx)) is dead far more often than 64 consecutive pixels of the flattened map, a 64 x 1 strip
// wrapped over two rows.  Every cost is computed per pixel by its own lane, so the map changes no bit of any result.
// Lanes past the image (a ragged right / bottom tile; the tail of the flattened map) are inactive: their x and y are
// clamped separately for their loads, they do not vote in the dead-view ballot and they store nothing.
__device__ __forceinline__ bool sr_mlp_lane_pixel(const SrMlpParams& p, int tile, int lane, int& y, int& x) {
  if (p.tiles_x) {
    const int ty = tile / p.tiles_x, tx = tile - ty * p.tiles_x;   // wave-uniform
    const int ly = (ty << p.th_log2) + (lane >> p.tw_log2);
    const int lx = (tx << p.tw_log2) + (lane & ((1 << p.tw_log2) - 1));
    y = min(ly, p.h - 1);
    x = min(lx, p.w - 1);
    return ly < p.h && lx < p.w;
  }
  const int N = p.h * p.w, pix = tile * 64 + lane;
  const int pc = min(pix, N - 1);
  y = pc / p.w;
  x = pc - y * p.w;
  return pix < N;
}

__device__ __forceinline__ void sr_swap_halves(float fa, float fb, float& bP, float& bQ) {
  // vdst lanes 32-63 <-> src lanes 0-31: bP = [fa(0..31) | fb(0..31)], bQ = [fa(32..63) | fb(32..63)]
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(fa), __float_as_uint(fb), false, false);
  bP = __uint_as_float(r[0]);
  bQ = __uint_as_float(r[1]);
}

#define SR_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ void sr_l1_step(f32x16 (&acc)[2][4], const float4 wA, float fa, float fb) {
  float bP, bQ;
  sr_swap_halves(fa, fb, bP, bQ);
  acc[0][0] = SR_MFMA(wA.x, bP, acc[0][0]);
  acc[1][0] = SR_MFMA(wA.x, bQ, acc[1][0]);
  acc[0][1] = SR_MFMA(wA.y, bP, acc[0][1]);
  acc[1][1] = SR_MFMA(wA.y, bQ, acc[1][1]);
  acc[0][2] = SR_MFMA(wA.z, bP, acc[0][2]);
  acc[1][2] = SR_MFMA(wA.z, bQ, acc[1][2]);
  acc[0][3] = SR_MFMA(wA.w, bP, acc[0][3]);
  acc[1][3] = SR_MFMA(wA.w, bQ, acc[1][3]);
}

// first k-step of a plane: D = A*B + hc (the hoisted depth-invariant part), no accumulator copy
__device__ __forceinline__ void sr_l1_step_init(f32x16 (&acc)[2][4], const f32x16 (&hc)[2][4], const float4 wA,
                                                float fa, float fb) {
  float bP, bQ;
  sr_swap_halves(fa, fb, bP, bQ);
  acc[0][0] = SR_MFMA(wA.x, bP, hc[0][0]);
  acc[1][0] = SR_MFMA(wA.x, bQ, hc[1][0]);
  acc[0][1] = SR_MFMA(wA.y, bP, hc[0][1]);
  acc[1][1] = SR_MFMA(wA.y, bQ, hc[1][1]);
  acc[0][2] = SR_MFMA(wA.z, bP, hc[0][2]);
  acc[1][2] = SR_MFMA(wA.z, bQ, hc[1][2]);
  acc[0][3] = SR_MFMA(wA.w, bP, hc[0][3]);
  acc[1][3] = SR_MFMA(wA.w, bQ, hc[1][3]);
}

// a wave-uniform flag in a scalar register whose value the optimiser cannot see through
__device__ __forceinline__ int sr_opaque(bool flag) {
  int v = __builtin_amdgcn_readfirstlane((int)flag);
  asm volatile("" : "+s"(v));
  return v;
}

#define SR_LDS_W3_FLOATS 256  // w3tab (128) + b3 + pad, in front of W1 in LDS

// ---- stages shared by sr_mlp_volume_kernel and sr_mlp_volume_split_kernel ----

// current-frame ray F.normalize(X) (cost_volume.py:641-651, eps 1e-12): X = d * r, so the ray does not depend
// on the plane beyond rounding; it is formed from plane 0 (depth d0) for every chunk (so results do not depend on how
// planes are chunked into work units) and shared by all planes.  crn: cosine_similarity's first operand.
__device__ __forceinline__ void sr_mlp_cur_ray(float d0, float r0, float r1, float r2, float& cr0, float& cr1, float& cr2,
                                               float& crn0, float& crn1, float& crn2) {
#pragma clang fp contract(off)
  const float X0 = d0 * r0, X1 = d0 * r1, X2 = d0 * r2;
  const float cden = fmaxf(sqrtf((X0 * X0 + X1 * X1) + X2 * X2), 1e-12f);
  cr0 = X0 / cden; cr1 = X1 / cden; cr2 = X2 / cden;
  const float n1 = fmaxf(sqrtf((cr0 * cr0 + cr1 * cr1) + cr2 * cr2), 1e-5f);
  crn0 = cr0 / n1; crn1 = cr1 / n1; crn2 = cr2 / n1;
}

// the four bilinear taps of a sample, 16 channels each, from the channels-last image `img`
__device__ __forceinline__ void sr_mlp_load_taps(const float* img, const SrSample& smp, float4 (&taps)[16]) {
  const float4* t_nw = reinterpret_cast<const float4*>(img + (size_t)smp.o_nw * 16);
  const float4* t_ne = reinterpret_cast<const float4*>(img + (size_t)smp.o_ne * 16);
  const float4* t_sw = reinterpret_cast<const float4*>(img + (size_t)smp.o_sw * 16);
  const float4* t_se = reinterpret_cast<const float4*>(img + (size_t)smp.o_se * 16);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    taps[i] = t_nw[i]; taps[4 + i] = t_ne[i]; taps[8 + i] = t_sw[i]; taps[12 + i] = t_se[i];
  }
}

template <bool W1_LDS, bool W2_LDS>
__global__ __launch_bounds__(256, 1) void sr_mlp_volume_kernel(SrMlpParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int C = 16;
  constexpr int VS = SR_VIEW_SLOTS / 2;  // k-steps per view
  const int lane = threadIdx.x & 63;
  const int steps_var = VS * p.K;
  const int steps1 = steps_var + (SR_INV_FIXED + 3 * p.K + 1) / 2;
  const float4* gW1 = reinterpret_cast<const float4*>(p.packed);
  const float4* gW1inv = gW1 + (size_t)steps_var * 64;
  const float4* gW2 = gW1 + (size_t)steps1 * 64;
  const float* gW3 = p.packed + (size_t)(steps1 + SR_MLP_STEPS2) * 256;

  for (int i = threadIdx.x; i < 129; i += blockDim.x) lds[i] = gW3[i];
  // LDS: [w3tab + b3 | W2 (65 KB, when it fits) | depth-variant part of W1 (12*K KB, when it fits)]
  constexpr int W2_FLOATS = W2_LDS ? SR_MLP_STEPS2 * 256 : 0;
  if (W2_LDS) {
    float4* l4 = reinterpret_cast<float4*>(lds + SR_LDS_W3_FLOATS);
    for (int i = threadIdx.x; i < SR_MLP_STEPS2 * 64; i += blockDim.x) l4[i] = gW2[i];
  }
  if (W1_LDS) {
    float4* l4 = reinterpret_cast<float4*>(lds + SR_LDS_W3_FLOATS + W2_FLOATS);
    for (int i = threadIdx.x; i < steps_var * 64; i += blockDim.x) l4[i] = gW1[i];
  }
  __syncthreads();
  const float4* W1p = W1_LDS ? reinterpret_cast<const float4*>(lds + SR_LDS_W3_FLOATS + W2_FLOATS) : gW1;

  const int N = p.h * p.w;
  const long nunits = (long)p.B * p.tiles * p.chunks;
  // XCD-aware work order (r04): workgroup b runs on XCD b % 8 and each XCD has its own 4 MB L2.  With units dealt round-robin
  // every XCD touches every region of every source image (41 MB per keyframe at 15 views) and the tap reads miss its L2
  // again and again (r03 PMC, cfg5: 1.2 GB of fabric traffic per launch for 244 MB of compulsory bytes).  Units are
  // ordered (image, pixel tile, plane chunk): give XCD x the contiguous eighth [x U8, (x + 1) U8) -- a band of pixel tiles
  // whose tap footprints overlap -- and let its waves stride through that band.
  constexpr int WPB = 4;  // waves per block: every launch is 256 threads (__launch_bounds__, SR_MLP_LAUNCH)
  // (the wave index as a scalar: units, planes and views then loop under scalar branches, and the dead-view bodies below are
  // selected by plain s_cbranch instead of being flattened into a predicated chain)
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  long wave0 = (long)blockIdx.x * WPB + wid;
  long nwaves = (long)gridDim.x * WPB;
  long unit_end = nunits;
  if ((gridDim.x & 7) == 0) {
    const long u8 = (nunits + 7) / 8;
    const int xcd = blockIdx.x & 7;
    nwaves = (long)(gridDim.x >> 3) * WPB;
    wave0 = xcd * u8 + (long)(blockIdx.x >> 3) * WPB + wid;
    unit_end = min(nunits, (xcd + 1) * u8);
  }
  const int half = lane >> 5;

  // A wave strides through the units by nwaves, usually a multiple of the chunk count: it would own the SAME plane chunk of
  // every pixel tile it visits.  Planes no longer cost the same (near planes have the most dead views, see below), and the
  // waves of the far chunks would finish last with everybody else idle.  So the chunk of a unit is rotated by the number
  // of strides that lead to it: per pixel tile still every chunk exactly once, per wave every chunk in turn.
  const int rot = (int)max(1L, nwaves / p.chunks);
  for (long unit = wave0; unit < unit_end; unit += nwaves) {
    const long tb = unit / p.chunks;
    const int chunk = (int)((unit % p.chunks + tb / rot) % p.chunks);
    const int tile = (int)(tb % p.tiles);
    const int b = (int)(tb / p.tiles);
    const int j0 = chunk * p.chunk, j1 = min(p.D, j0 + p.chunk);
    int y, x;
    const bool in_image = sr_mlp_lane_pixel(p, tile, lane, y, x);
    const int pc = y * p.w + x;             // this lane's pixel, clamped into the image: what it loads from
    const int pix = in_image ? pc : -1;     // ... and what it stores to; one register carries both pixel and activity
    const bool active = pix >= 0;
    const float* plane_ptr = p.planes.ptr + b * p.planes.sb + y * p.planes.sy + x * p.planes.sx;
    const float* geom_b = p.geom + (size_t)b * p.K * SR_GEOM_STRIDE;
    const float* src_b = p.src_nhwc + (size_t)b * p.K * N * C;

    float cur[C];
    if (p.cur_nhwc) {   // (wave-uniform) the same 16 values either way
      const float4* c4 = reinterpret_cast<const float4*>(p.cur + ((size_t)b * N + pc) * C);
#pragma unroll
      for (int i = 0; i < C / 4; ++i) {
        const float4 v = c4[i];
        cur[4 * i] = v.x; cur[4 * i + 1] = v.y; cur[4 * i + 2] = v.z; cur[4 * i + 3] = v.w;
      }
    } else {
#pragma unroll
      for (int c = 0; c < C; ++c) cur[c] = p.cur[((size_t)b * C + c) * N + pc];
    }

    float r0, r1, r2;
    sr_pixel_ray(p.invK + 16 * (size_t)b, x, y, r0, r1, r2);
    float cr0, cr1, cr2, crn0, crn1, crn2;
    sr_mlp_cur_ray(plane_ptr[0], r0, r1, r2, cr0, cr1, cr2, crn0, crn1, crn2);

    // ---- depth-invariant part of layer 1 (weights straight from L2, once per unit) ----
    f32x16 hc[2][4];
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) hc[g][m][r] = 0.0f;
    {
      const float4* wi = gW1inv + lane;
#pragma unroll
      for (int t = 0; t < 8; ++t) sr_l1_step(hc, wi[t * 64], cur[2 * t], cur[2 * t + 1]);
      sr_l1_step(hc, wi[8 * 64], cr0, cr1);
      sr_l1_step(hc, wi[9 * 64], cr2, 1.0f);
      const int npose = 3 * p.K;
#pragma unroll 1
      for (int u = 0; u < npose; u += 2) {  // pose measures: [b,k] scalars (geometry_utils.py:178-191)
        const int ka = u / 3, ia = u - 3 * ka, kb = (u + 1) / 3, ib = (u + 1) - 3 * kb;
        const float fa = geom_b[ka * SR_GEOM_STRIDE + 15 + ia];
        const float fb = (u + 1 < npose) ? geom_b[kb * SR_GEOM_STRIDE + 15 + ib] : 0.0f;
        sr_l1_step(hc, wi[(size_t)(10 + (u >> 1)) * 64], fa, fb);
      }
    }

    SrSample smp;
    float4 taps[16];
    float X0, X1, X2, d;
    bool any_depth, any_bounds;
    // A view is DEAD for this wave at this plane when no tap of any of its pixels lies inside the source image: its 16
    // warped channels and dot * mask are exact zeros (zeros padding), so its feature k-steps 0..7 would add W . 0 and its
    // tap loads, interpolation and dot product would only produce those zeros.  Wave-uniform (a ballot), keyed on the
    // tap validity tests and not on z' > 0: a point behind the camera has mask 0, but its mirrored taps can be in the
    // image and the reference does not mask the warped features by depth.  The clamped lanes of a ragged tile
    // (sr_mlp_lane_pixel) do not vote; what they compute is never stored.
    // (the view's camera centre is read here, in front of its tap loads: vector loads return in order, and read behind
    // them it made the first k-step wait for all 16 taps)
    float gt0, gt1, gt2;
    auto project_view = [&](int k) -> bool {
      const float* g = geom_b + k * SR_GEOM_STRIDE;
      gt0 = g[12]; gt1 = g[13]; gt2 = g[14];
      sr_project_sample(g, X0, X1, X2, p.h, p.w, p.inv_w, p.inv_h, smp);
      return __builtin_amdgcn_ballot_w64(active & smp.any_tap) == 0;
    };
    auto load_taps = [&](int k) {
      sr_mlp_load_taps(src_b + (size_t)k * N * C, smp, taps);
    };
    // pieces of the per-view feature assembly (o = fn or f); the ray pieces need no taps
    float rv0, rv1, rv2, rsd, rdot;
#define SR_RAY_A_T(t0, t1, t2)                                                                \
    {                                                                                         \
      _Pragma("clang fp contract(off)")                                                       \
      rv0 = X0 - (t0); rv1 = X1 - (t1); rv2 = X2 - (t2);                                       \
      rsd = fmaxf(sqrtf((rv0 * rv0 + rv1 * rv1) + rv2 * rv2), 1e-12f);                         \
    }
#define SR_RAY_A(o, g, kview)  /* the split kernel: every view carries its spare slot */      \
    SR_RAY_A_T((g)[12], (g)[13], (g)[14]) (o)[23] = ((kview) == 0) ? d : 0.0f;
#define SR_RAY_A0 SR_RAY_A_T(gt0, gt1, gt2)  /* camera centre read by project_view */
  // (r03) the source ray F.normalize(X - t_k) (cost_volume.py:654-669) and the ray angle F.cosine_similarity(...)
  // (:683-688) divide three components by one norm each: ONE IEEE reciprocal + three multiplies per normalisation
  // instead of three IEEE divisions (10 VALU instructions apiece beside the MFMAs).  x * (1/n) differs from x / n by at
  // most one ulp; these channels only feed the MLP (parity bar 1e-4, tests: 2e-5 vs the oracle's true divisions).
#define SR_RAY_B(o)                                                                           \
    {                                                                                         \
      _Pragma("clang fp contract(off)")                                                       \
      const float rinv = 1.0f / rsd;                                                          \
      (o)[19] = rv0 * rinv; (o)[20] = rv1 * rinv; (o)[21] = rv2 * rinv;                        \
    }
#define SR_RAY_C(o)                                                                           \
    {                                                                                         \
      _Pragma("clang fp contract(off)")                                                       \
      const float n2 = fmaxf(sqrtf(((o)[19] * (o)[19] + (o)[20] * (o)[20]) + (o)[21] * (o)[21]), 1e-5f); \
      (o)[18] = ((crn0 * (o)[19] + crn1 * (o)[20]) + crn2 * (o)[21]) * (1.0f / n2);            \
    }
#define SR_INTERP2(o, i, lo)  /* channels 4i+2lo, 4i+2lo+1 as one packed fp32 pair (v_pk_fma_f32) */       \
    {                                                                                         \
      const float4 a = taps[i], bq = taps[4 + (i)], c4 = taps[8 + (i)], d4 = taps[12 + (i)];   \
      const sr_f2v ta = (lo) == 0 ? sr_f2v{a.x, a.y} : sr_f2v{a.z, a.w};                       \
      const sr_f2v tb = (lo) == 0 ? sr_f2v{bq.x, bq.y} : sr_f2v{bq.z, bq.w};                   \
      const sr_f2v tc = (lo) == 0 ? sr_f2v{c4.x, c4.y} : sr_f2v{c4.z, c4.w};                   \
      const sr_f2v td = (lo) == 0 ? sr_f2v{d4.x, d4.y} : sr_f2v{d4.z, d4.w};                   \
      const sr_f2v r2 = __builtin_elementwise_fma(sr_f2v{smp.w_se, smp.w_se}, td,              \
                        __builtin_elementwise_fma(sr_f2v{smp.w_sw, smp.w_sw}, tc,              \
                        __builtin_elementwise_fma(sr_f2v{smp.w_ne, smp.w_ne}, tb,              \
                                                  sr_f2v{smp.w_nw, smp.w_nw} * ta)));          \
      (o)[4 * (i) + 2 * (lo) + 0] = r2.x;                                                     \
      (o)[4 * (i) + 2 * (lo) + 1] = r2.y;                                                     \
    }
#define SR_DOT(o)                                                                             \
    {                                                                                         \
      rdot = 0.0f;                                                                            \
      _Pragma("unroll") for (int c = 0; c < 16; ++c) rdot = fmaf((o)[c], cur[c], rdot);        \
      const bool front = smp.zp > 0.0f;                                                       \
      any_depth |= front;                                                                     \
      any_bounds |= sr_in_bounds(smp, p.h, p.w);                                              \
      (o)[16] = front ? 1.0f : 0.0f; /* mask (cost_volume.py:611-612) */                      \
      (o)[17] = smp.zp;              /* z'_k (cost_volume.py:603-609) */                      \
      (o)[22] = front ? rdot : 0.0f; /* dot * mask (cost_volume.py:691-695) */                \
    }
#define SR_DOT_DEAD(o)  /* SR_DOT of a dead view: channels 0..15 are never read, dot * mask is 0 */ \
    {                                                                                         \
      const bool front = smp.zp > 0.0f;                                                       \
      any_depth |= front;                                                                     \
      any_bounds |= sr_in_bounds(smp, p.h, p.w);                                              \
      (o)[16] = front ? 1.0f : 0.0f;                                                          \
      (o)[17] = smp.zp;                                                                       \
      (o)[22] = 0.0f;                                                                         \
    }
#define SR_SB __builtin_amdgcn_sched_barrier(0);

    // costs of this unit's planes, kept until the 16-byte stores at its end: in registers (select chain), or -- in the
    // variants that stream W1 and have neither registers nor a full LDS -- in a wave-private LDS strip
    constexpr bool CST_LDS = !W1_LDS;
    const int cst_base = SR_LDS_W3_FLOATS + W2_FLOATS +
                         wid * (SR_PLANE_CHUNK * 64);   // scalar
    float cst[SR_PLANE_CHUNK];
#pragma unroll
    for (int q = 0; q < SR_PLANE_CHUNK; ++q) cst[q] = 0.0f;
#pragma unroll 1
    for (int j = j0; j < j1; ++j) {
      d = plane_ptr[j * p.planes.sd];
      {
#pragma clang fp contract(off)
        X0 = d * r0; X1 = d * r1; X2 = d * r2;  // geometry_utils.py:56-57
      }
      any_depth = false; any_bounds = false;
      f32x16 acc[2][4];
      // per plane, so that the channels a dead view leaves unwritten (and nobody reads) are not live across layer 2
      float f[SR_VIEW_SLOTS], fn[SR_VIEW_SLOTS];

      bool dc = project_view(0), dn;  // is the view being multiplied / being assembled dead?
      if (!dc) {  // view 0, not overlapped
        load_taps(0);
        SR_RAY_A0 SR_RAY_B(f) SR_RAY_C(f)
        SR_INTERP2(f, 0, 0) SR_INTERP2(f, 0, 1) SR_INTERP2(f, 1, 0) SR_INTERP2(f, 1, 1)
        SR_INTERP2(f, 2, 0) SR_INTERP2(f, 2, 1) SR_INTERP2(f, 3, 0) SR_INTERP2(f, 3, 1)
        SR_DOT(f)
      } else {
        SR_RAY_A0 SR_RAY_B(f) SR_RAY_C(f)
        SR_DOT_DEAD(f)
        f[0] = f[1] = 0.0f;  // named (not used) by the select in front of the first step
      }
      // ---- layer 1, software-pipelined over views: the feature vector of view k+1 is assembled in small VALU
      // pieces, each placed in the shadow of one k-step (8 MFMAs = 512 cycles) of view k; its 16 tap loads are
      // issued before the first step.  sched_barrier(0) pins the placement.  Four straight-line bodies, selected by
      // scalar branches per view (so every tap load is consumed inside the body that issued it and no s_waitcnt has to
      // be pessimistic behind a join):
      //   view k live: steps 0..11; the taps of view k+1 are first touched at step 7 (>= 3.5k cycles after issue)
      //   view k dead: steps 8..10 only (slots 16..21: mask, z', ray angle, rays); step 11 would multiply dot * mask and
      //                the spare slot, exact zeros both (SR_DOT_DEAD; no W1 column and no value for k > 0: sr_mlp_var_col,
      //                SR_RAY_A_T) -- except for view 0, whose spare slot carries the plane depth: it keeps step 11.  The
      //                taps of view k+1 are first touched at step 10, two k-steps after their issue
      //   view k+1 dead: no tap loads, no interpolation, no dot product
      // The executed k-steps keep their ascending (view, step) order, so every accumulator sees the same sequence of
      // non-zero additions as without the skip.  The last iteration has no view k+1: it re-derives the metadata of
      // view K-1 as a dead view (any_depth / any_bounds are ORs: idempotent), nothing reads it.
      // The first executed step of view 0 takes the hoisted invariant part as its C operand (no accumulator copy).
#define SR_STEP(t)                                           \
        wN = wk[((t) + 1 < VS ? (t) + 1 : (t)) * 64];       \
        sr_l1_step(acc, wA, f[2 * (t)], f[2 * (t) + 1]);     \
        wA = wN;
#define SR_STEP11(FIRST)  /* the spare slot: the plane depth for view 0, nothing (0) for every other view */ \
        sr_l1_step(acc, wA, f[22], (FIRST) ? d : 0.0f);
#define SR_STEP_END(t) sr_l1_step(acc, wA, f[2 * (t)], f[2 * (t) + 1]);  /* the body's last step: no next weights */
#define SR_IF_LIVE(ND, x) if (!(ND)) { x }
#define SR_VIEW_BODY(FIRST, CD, ND)                                                    \
        {                                                                              \
          if (!(ND)) load_taps(kn);                                                    \
          const float4* wk = W1p + (size_t)(VS * k) * 64 + lane;                       \
          float4 wA = wk[((CD) ? 8 : 0) * 64 + ((FIRST) ? 64 : 0)], wN;                \
          SR_SB                                                                        \
          if (!(CD)) {                                                                 \
            if (!(FIRST)) { SR_STEP(0) SR_RAY_A0 SR_SB }                     \
            SR_STEP(1) if (FIRST) { SR_RAY_A0 } SR_RAY_B(fn) SR_SB           \
            SR_STEP(2) SR_RAY_C(fn) SR_SB                                              \
            SR_STEP(3) SR_SB                                                           \
            SR_STEP(4) SR_SB                                                           \
            SR_STEP(5) SR_SB                                                           \
            SR_STEP(6) SR_SB                                                           \
            SR_STEP(7) SR_IF_LIVE(ND, SR_INTERP2(fn, 0, 0) SR_INTERP2(fn, 0, 1)) SR_SB \
            SR_STEP(8) SR_IF_LIVE(ND, SR_INTERP2(fn, 1, 0) SR_INTERP2(fn, 1, 1)) SR_SB \
            SR_STEP(9) SR_IF_LIVE(ND, SR_INTERP2(fn, 2, 0) SR_INTERP2(fn, 2, 1)) SR_SB \
            SR_STEP(10) SR_IF_LIVE(ND, SR_INTERP2(fn, 3, 0)) SR_SB                     \
            SR_STEP11(FIRST) if (ND) { SR_DOT_DEAD(fn) } else { SR_INTERP2(fn, 3, 1) SR_DOT(fn) } SR_SB \
          } else if (FIRST) {  /* dead view 0: step 8 ran in front of the bodies, step 11 carries the plane depth */ \
            SR_STEP(9) SR_RAY_A0 SR_RAY_B(fn) SR_RAY_C(fn) SR_SB               \
            SR_STEP(10) SR_IF_LIVE(ND, SR_INTERP2(fn, 0, 0) SR_INTERP2(fn, 0, 1)       \
                                       SR_INTERP2(fn, 1, 0) SR_INTERP2(fn, 1, 1)) SR_SB \
            SR_STEP11(FIRST) if (ND) { SR_DOT_DEAD(fn) } else {                             \
              SR_INTERP2(fn, 2, 0) SR_INTERP2(fn, 2, 1) SR_INTERP2(fn, 3, 0) SR_INTERP2(fn, 3, 1) SR_DOT(fn) } SR_SB \
          } else {             /* dead view k > 0: three steps */                      \
            SR_STEP(8) SR_RAY_A0 SR_SB                                         \
            SR_STEP(9) SR_RAY_B(fn) SR_RAY_C(fn) SR_SB                                 \
            SR_STEP_END(10) if (ND) { SR_DOT_DEAD(fn) } else {                         \
              SR_INTERP2(fn, 0, 0) SR_INTERP2(fn, 0, 1) SR_INTERP2(fn, 1, 0) SR_INTERP2(fn, 1, 1) SR_SB \
              SR_INTERP2(fn, 2, 0) SR_INTERP2(fn, 2, 1) SR_INTERP2(fn, 3, 0) SR_INTERP2(fn, 3, 1) SR_DOT(fn) } SR_SB \
          }                                                                            \
          _Pragma("unroll") for (int t = (ND) ? 16 : 0; t < SR_VIEW_SLOTS - 1; ++t) f[t] = fn[t]; \
        }
      // The four bodies are four if-without-else in a row on four flags the compiler cannot relate to each other
      // (sr_opaque): hipcc flattens an if / else between live accumulators into a predicated chain whose joins carry
      // undefined accumulator values, and then copies (128 v_accvgpr_mov per view) and spills them.
#define SR_VIEW(FIRST)                                                                 \
        {                                                                              \
          const int kn = min(k + 1, p.K - 1);                                          \
          dn = project_view(kn) | (k + 1 >= p.K);                                      \
          const int ll = sr_opaque(!dc & !dn), ld = sr_opaque(!dc & dn);               \
          const int dl = sr_opaque(dc & !dn), dd = sr_opaque(dc & dn);                 \
          if (ll) SR_VIEW_BODY(FIRST, false, false)                                    \
          if (ld) SR_VIEW_BODY(FIRST, false, true)                                     \
          if (dl) SR_VIEW_BODY(FIRST, true, false)                                     \
          if (dd) SR_VIEW_BODY(FIRST, true, true)                                      \
          dc = dn;                                                                     \
        }
      {  // the first executed step of view 0 (step 0, or step 8 when the view is dead) takes the hoisted invariant part
         // as its C operand: no accumulator copy.  ONE site for both cases, outside the bodies below: with the
         // step that reads hc under a branch, hipcc evicts hc around layer 2 (80 accumulators to scratch per plane).
        const float4 w0 = W1p[(size_t)(dc ? 8 * 64 : 0) + lane];
        sr_l1_step_init(acc, hc, w0, dc ? f[16] : f[0], dc ? f[17] : f[1]);
      }
      {
        const int k = 0;
        SR_VIEW(true)
      }
#pragma unroll 1
      for (int k = 1; k < p.K; ++k) SR_VIEW(false)

      // layer 2: the layer-1 accumulators, passed through LeakyReLU(slope) = max(v, slope*v) (networks.py:139,
      // 0 < slope < 1) on the fly, are the B operands; W2 streams from L2 three steps ahead
      // (not zeroed: the first k-step takes the constant 0 as its C operand -- 128 v_mov per plane and wave otherwise)
      f32x16 acc2[2][4];
      const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      const float4* w2 = (W2_LDS ? reinterpret_cast<const float4*>(lds + SR_LDS_W3_FLOATS) : gW2) + lane;
      if (!W2_LDS) asm volatile("" : "+v"(w2));  // keep hipcc from hoisting 65 loop-invariant 64-bit addresses (spills)
      float4 wn0 = w2[0], wn1 = w2[64], wn2 = w2[128];
#pragma unroll
      for (int t = 0; t < 64; ++t) {
        const float4 wA = wn0;
        wn0 = wn1;
        wn1 = wn2;
        wn2 = w2[(size_t)min(t + 3, 64) * 64];
        const float aP = acc[0][t >> 4][t & 15], aQ = acc[1][t >> 4][t & 15];
        const float bP = sr_vmax_mfma(aP, p.slope * aP), bQ = sr_vmax_mfma(aQ, p.slope * aQ);
        acc2[0][0] = SR_MFMA(wA.x, bP, t == 0 ? zero16 : acc2[0][0]);
        acc2[1][0] = SR_MFMA(wA.x, bQ, t == 0 ? zero16 : acc2[1][0]);
        acc2[0][1] = SR_MFMA(wA.y, bP, t == 0 ? zero16 : acc2[0][1]);
        acc2[1][1] = SR_MFMA(wA.y, bQ, t == 0 ? zero16 : acc2[1][1]);
        acc2[0][2] = SR_MFMA(wA.z, bP, t == 0 ? zero16 : acc2[0][2]);
        acc2[1][2] = SR_MFMA(wA.z, bQ, t == 0 ? zero16 : acc2[1][2]);
        acc2[0][3] = SR_MFMA(wA.w, bP, t == 0 ? zero16 : acc2[0][3]);
        acc2[1][3] = SR_MFMA(wA.w, bQ, t == 0 ? zero16 : acc2[1][3]);
      }
      {
        const float4 wA = wn0;  // bias step (t = 64)
        const float one = half ? 0.0f : 1.0f;
        acc2[0][0] = SR_MFMA(wA.x, one, acc2[0][0]);
        acc2[1][0] = SR_MFMA(wA.x, one, acc2[1][0]);
        acc2[0][1] = SR_MFMA(wA.y, one, acc2[0][1]);
        acc2[1][1] = SR_MFMA(wA.y, one, acc2[1][1]);
        acc2[0][2] = SR_MFMA(wA.z, one, acc2[0][2]);
        acc2[1][2] = SR_MFMA(wA.z, one, acc2[1][2]);
        acc2[0][3] = SR_MFMA(wA.w, one, acc2[0][3]);
        acc2[1][3] = SR_MFMA(wA.w, one, acc2[1][3]);
      }

      // layer 3 (128 -> 1, no activation: disable_final_activation=True, cost_volume.py:438); w3tab in LDS
      const float4* w3 = reinterpret_cast<const float4*>(lds + half * 64);
      sr_f2v oPQ = {0.0f, 0.0f};  // the two point groups as one packed fp32 pair (v_pk_mul_f32 / v_pk_fma_f32)
      const sr_f2v slope2 = {p.slope, p.slope};
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 wv = w3[m * 4 + q];
          const float wr[4] = {wv.x, wv.y, wv.z, wv.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const sr_f2v h2 = {acc2[0][m][4 * q + i], acc2[1][m][4 * q + i]};
            const sr_f2v s2 = slope2 * h2;
            oPQ = __builtin_elementwise_fma(sr_f2v{wr[i], wr[i]}, sr_f2v{sr_vmax(h2.x, s2.x), sr_vmax(h2.y, s2.y)}, oPQ);
          }
        }
      float oP = oPQ.x, oQ = oPQ.y;
      oP += __shfl_xor(oP, 32);
      oQ += __shfl_xor(oQ, 32);
      const float cost = (half ? oQ : oP) + lds[128];

      if (p.vec_store) {
        if (CST_LDS) lds[cst_base + (j - j0) * 64 + lane] = cost;
        else {
#pragma unroll
          for (int q = 0; q < SR_PLANE_CHUNK; ++q) cst[q] = (j - j0 == q) ? cost : cst[q];
        }
      }
      if (active) {
        if (!p.vec_store) p.out.cv[b * p.out.sb + j * p.out.sd + (int64_t)pix * p.out.sp] = cost;
        if (j == p.D - 1 && p.out.mask) p.out.mask[(size_t)b * N + pix] = (uint8_t)(any_depth && any_bounds);
      }
    }
    if (p.vec_store && active) {   // planes j0 .. j1-1 of this pixel are consecutive floats (host checked the alignment)
      float* row = p.out.cv + b * p.out.sb + (int64_t)pix * p.out.sp + j0;
      if (CST_LDS) {
#pragma unroll
        for (int q = 0; q < SR_PLANE_CHUNK; ++q) cst[q] = lds[cst_base + q * 64 + lane];   // this lane's own writes: no barrier
      }
#pragma unroll
      for (int q = 0; q < SR_PLANE_CHUNK; q += 4) {
        if (j0 + q + 4 <= j1) *reinterpret_cast<float4*>(row + q) = make_float4(cst[q], cst[q + 1], cst[q + 2], cst[q + 3]);
        else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (j0 + q + i < j1) row[q + i] = cst[q + i];
        }
      }
    }
  }
}

// ------------------------------------------------------------------ split-precision variant (fenced experiment) ----
// SR_MLP_SPLIT=bf16|f16 (read per call; default off): layers 1 (depth-variant part) and 2 run on the 16-bit matrix pipe
// (v_mfma_f32_32x32x16_{bf16,f16}: 16x the fp32 rate) with every fp32 operand split into two 16-bit pieces,
// x = x_hi + x_lo (round-to-nearest each), and three products per k-step, x_hi w_hi + x_hi w_lo + x_lo w_hi, accumulated in
// fp32 by the MFMA (the dropped x_lo w_lo term is 2^-18 (bf16) / 2^-24 (f16) of the product).  Inputs, outputs, the
// depth-invariant part of layer 1, layer 3 and every accumulator stay fp32.  Same wave-owns-64-points structure as the
// fp32 kernel; a k-step now covers 16 inputs (8 per half-wave), so a view is two steps: its 16 warped channels, then its 8
// metadata slots (upper k-half zero).  The layer-1 accumulators still ARE the layer-2 B operands (after LeakyReLU and
// the split).  Not the default and not what bench.py's headline measures.

template <int FMT> struct SrSplitFmt;
template <> struct SrSplitFmt<1> {   // two bf16 pieces: 16-17 significant bits, fp32 exponent range
  typedef __bf16 e2 __attribute__((ext_vector_type(2)));
  typedef __bf16 e8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ void split(float a, float b, unsigned& hi, unsigned& lo) {
    const sr_f2v v = {a, b};
    hi = __builtin_bit_cast(unsigned, __builtin_convertvector(v, e2));
    const sr_f2v v0 = {__uint_as_float(hi << 16), __uint_as_float(hi & 0xffff0000u)};
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(v - v0, e2));
  }
  static __device__ __forceinline__ f32x16 mfma(sr_u4 a, sr_u4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(e8, a), __builtin_bit_cast(e8, b), c, 0, 0, 0);
  }
};
template <> struct SrSplitFmt<2> {   // two fp16 pieces: 22-24 significant bits for 2^-14 <= |x| < 65504 (denormal pieces are
  typedef _Float16 e2 __attribute__((ext_vector_type(2)));   // honoured by v_cvt_pk_f16_f32 and the MFMA: measured on gfx950);
  typedef _Float16 e8 __attribute__((ext_vector_type(8)));   // beyond +-65504 the high piece is inf and the result NaN -- loud,
  static __device__ __forceinline__ void split(float a, float b, unsigned& hi, unsigned& lo) {   // not a saturated wrong value
    const sr_f2v v = {a, b};
    const e2 h = __builtin_convertvector(v, e2);
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(v - __builtin_convertvector(h, sr_f2v), e2));
  }
  static __device__ __forceinline__ f32x16 mfma(sr_u4 a, sr_u4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(e8, a), __builtin_bit_cast(e8, b), c, 0, 0, 0);
  }
};

// LDS / packed layout of the split variant (32-bit words):
//   table  [0,512):   w3tab (128) | b3 (1) | pad | b2tab at 256 (128: C layout, [half][mt][r])
//   W2     8 steps x [mt 4][piece 2][lane 64][4 words]                        = 16384 words
//   W1var  per view: step A [mt 4][piece 2][lane 64][4] (2048) + metadata step [mt 4][piece 2][lane 32][4] (1024)
#define SR_SPL_TAB 512
#define SR_SPL_W2_WORDS 16384
#define SR_SPL_VIEW_WORDS 3072

template <int FMT>
__global__ void sr_mlp_pack_split_kernel(const float* __restrict__ W1, const float* __restrict__ b1,
                                         const float* __restrict__ W2, const float* __restrict__ b2,
                                         const float* __restrict__ W3, const float* __restrict__ b3,
                                         float* __restrict__ packed, int K, int C) {
  typedef SrSplitFmt<FMT> S;
  const int steps_var = (SR_VIEW_SLOTS / 2) * K;
  const int steps_inv = (SR_INV_FIXED + 3 * K + 1) / 2;
  const int steps1 = steps_var + steps_inv;
  const int Cin = C * (K + 1) + 10 * K + 4;
  unsigned* pk = reinterpret_cast<unsigned*>(packed);
  auto put = [&](size_t word, int piece, float wa, float wb) {
    unsigned hi, lo;
    S::split(wa, wb, hi, lo);
    pk[word] = piece ? lo : hi;
  };
  const int total = (steps1 + SR_MLP_STEPS2) * 256 + 128 + 1;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    if (e < steps_var * 256) {
      const int k = e / SR_SPL_VIEW_WORDS, q = e - k * SR_SPL_VIEW_WORDS;
      int mt, piece, lane, dw, slot0;
      if (q < 2048) { mt = q >> 9; piece = (q >> 8) & 1; lane = (q >> 2) & 63; dw = q & 3; slot0 = 8 * (lane >> 5) + 2 * dw; }
      else { const int q2 = q - 2048; mt = q2 >> 8; piece = (q2 >> 7) & 1; lane = (q2 >> 2) & 31; dw = q2 & 3; slot0 = 16 + 2 * dw; }
      const int row = 32 * mt + (lane & 31);
      const int ca = sr_mlp_var_col(K, C, k, slot0), cb = sr_mlp_var_col(K, C, k, slot0 + 1);
      put(e, piece, ca >= 0 ? W1[(size_t)row * Cin + ca] : 0.0f, cb >= 0 ? W1[(size_t)row * Cin + cb] : 0.0f);
    } else if (e < steps1 * 256) {   // depth-invariant part: fp32, the layout of sr_mlp_pack_kernel
      const int e1 = e - steps_var * 256;
      const int t = e1 >> 8, lane = (e1 >> 2) & 63, mt = e1 & 3;
      const int row = 32 * mt + (lane & 31);
      const int col = sr_mlp_inv_col(K, C, 2 * t + (lane >> 5));
      packed[e] = (col >= 0) ? W1[(size_t)row * Cin + col] : (col == -2 ? b1[row] : 0.0f);
    } else if (e < steps1 * 256 + SR_SPL_W2_WORDS) {
      const int q = e - steps1 * 256;
      const int s = q >> 11, mt = (q >> 9) & 3, piece = (q >> 8) & 1, lane = (q >> 2) & 63, dw = q & 3;
      const int row = 32 * mt + (lane & 31);
      // k-slot (s, lane >> 5, i): the hidden feature held in accumulator register r = 8 (s & 1) + i of tile s >> 1
      auto feat = [&](int i) { const int r = 8 * (s & 1) + i; return 32 * (s >> 1) + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); };
      put(e, piece, W2[(size_t)row * SR_HID + feat(2 * dw)], W2[(size_t)row * SR_HID + feat(2 * dw + 1)]);
    } else if (e < (steps1 + SR_MLP_STEPS2) * 256) {
      const int i = e - steps1 * 256 - SR_SPL_W2_WORDS;   // 0..255: b2tab in the first 128
      const int half = i >> 6, mt = (i >> 4) & 3, r = i & 15;
      packed[e] = (i < 128) ? b2[32 * mt + (r & 3) + 8 * (r >> 2) + 4 * half] : 0.0f;
    } else if (e < (steps1 + SR_MLP_STEPS2) * 256 + 128) {
      const int i = e - (steps1 + SR_MLP_STEPS2) * 256;
      const int half = i >> 6, mt = (i >> 4) & 3, r = i & 15;
      packed[e] = W3[32 * mt + (r & 3) + 8 * (r >> 2) + 4 * half];
    } else {
      packed[e] = b3[0];
    }
  }
}

__device__ __forceinline__ void sr_swap_halves_u4(const sr_u4 fa, const sr_u4 fb, sr_u4& bP, sr_u4& bQ) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    auto r = __builtin_amdgcn_permlane32_swap(fa[i], fb[i], false, false);
    bP[i] = r[0];
    bQ[i] = r[1];
  }
}

// one 16-input k-step of layer 1 or 2: 4 output tiles x 2 point groups x 3 products
// INIT: 0 accumulate, 1 the first products take c0 as their C operand, 2 they take zero
template <int FMT, int INIT>
__device__ __forceinline__ void sr_spl_step(f32x16 (&acc)[2][4], const f32x16 (&c0)[2][4], const sr_u4* aw, int ls,
                                            const sr_u4 bPh, const sr_u4 bPl, const sr_u4 bQh, const sr_u4 bQl) {
  typedef SrSplitFmt<FMT> S;
  sr_u4 ah[4], al[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) { ah[m] = aw[(2 * m) * ls]; al[m] = aw[(2 * m + 1) * ls]; }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    acc[0][m] = S::mfma(ah[m], bPh, INIT == 1 ? c0[0][m] : (INIT == 2 ? zero16 : acc[0][m]));
    acc[1][m] = S::mfma(ah[m], bQh, INIT == 1 ? c0[1][m] : (INIT == 2 ? zero16 : acc[1][m]));
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    acc[0][m] = S::mfma(ah[m], bPl, acc[0][m]);
    acc[1][m] = S::mfma(ah[m], bQl, acc[1][m]);
  }
#pragma unroll
  for (int m = 0; m < 4; ++m) {
    acc[0][m] = S::mfma(al[m], bPh, acc[0][m]);
    acc[1][m] = S::mfma(al[m], bQh, acc[1][m]);
  }
}

template <int FMT>
__global__ __launch_bounds__(256, 1) void sr_mlp_volume_split_kernel(SrMlpParams p) {
  typedef SrSplitFmt<FMT> S;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  constexpr int C = 16;
  const int lane = threadIdx.x & 63;
  const int steps_var = (SR_VIEW_SLOTS / 2) * p.K;
  const int steps1 = steps_var + (SR_INV_FIXED + 3 * p.K + 1) / 2;
  const float4* gW1inv = reinterpret_cast<const float4*>(p.packed) + (size_t)steps_var * 64;
  const float* gW2 = p.packed + (size_t)steps1 * 256;
  const float* gW3 = p.packed + (size_t)(steps1 + SR_MLP_STEPS2) * 256;

  for (int i = threadIdx.x; i < 129; i += blockDim.x) lds[i] = gW3[i];
  for (int i = threadIdx.x; i < 128; i += blockDim.x) lds[256 + i] = gW2[SR_SPL_W2_WORDS + i];
  {
    float4* l4 = reinterpret_cast<float4*>(lds + SR_SPL_TAB);
    const float4* g4 = reinterpret_cast<const float4*>(gW2);
    for (int i = threadIdx.x; i < SR_SPL_W2_WORDS / 4; i += blockDim.x) l4[i] = g4[i];
    l4 += SR_SPL_W2_WORDS / 4;
    g4 = reinterpret_cast<const float4*>(p.packed);
    for (int i = threadIdx.x; i < p.K * (SR_SPL_VIEW_WORDS / 4); i += blockDim.x) l4[i] = g4[i];
  }
  __syncthreads();
  const sr_u4* W2s = reinterpret_cast<const sr_u4*>(lds + SR_SPL_TAB);
  const sr_u4* W1s = W2s + SR_SPL_W2_WORDS / 4;

  const int N = p.h * p.w;
  const long nunits = (long)p.B * p.tiles * p.chunks;
  long wave0 = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  long nwaves = (long)gridDim.x * (blockDim.x >> 6);
  long unit_end = nunits;
  if ((gridDim.x & 7) == 0) {   // XCD-contiguous unit ranges, as in sr_mlp_volume_kernel
    const long u8 = (nunits + 7) / 8;
    const int xcd = blockIdx.x & 7;
    nwaves = (long)(gridDim.x >> 3) * (blockDim.x >> 6);
    wave0 = xcd * u8 + (long)(blockIdx.x >> 3) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    unit_end = min(nunits, (xcd + 1) * u8);
  }
  const int half = lane >> 5;
  const sr_u4 zero4 = {0u, 0u, 0u, 0u};

  for (long unit = wave0; unit < unit_end; unit += nwaves) {
    const int chunk = (int)(unit % p.chunks);
    const long tb = unit / p.chunks;
    const int tile = (int)(tb % p.tiles);
    const int b = (int)(tb / p.tiles);
    const int j0 = chunk * p.chunk, j1 = min(p.D, j0 + p.chunk);
    int y, x;
    const bool in_image = sr_mlp_lane_pixel(p, tile, lane, y, x);
    const int pc = y * p.w + x;             // this lane's pixel, clamped into the image: what it loads from
    const int pix = in_image ? pc : -1;     // ... and what it stores to; one register carries both pixel and activity
    const bool active = pix >= 0;
    const float* plane_ptr = p.planes.ptr + b * p.planes.sb + y * p.planes.sy + x * p.planes.sx;
    const float* geom_b = p.geom + (size_t)b * p.K * SR_GEOM_STRIDE;
    const float* src_b = p.src_nhwc + (size_t)b * p.K * N * C;

    float cur[C];
#pragma unroll
    for (int c = 0; c < C; ++c) cur[c] = p.cur[((size_t)b * C + c) * N + pc];

    float r0, r1, r2;
    sr_pixel_ray(p.invK + 16 * (size_t)b, x, y, r0, r1, r2);
    float cr0, cr1, cr2, crn0, crn1, crn2;
    sr_mlp_cur_ray(plane_ptr[0], r0, r1, r2, cr0, cr1, cr2, crn0, crn1, crn2);

    // depth-invariant part of layer 1: fp32 MFMA, once per unit (as in sr_mlp_volume_kernel)
    f32x16 hc[2][4];
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) hc[g][m][r] = 0.0f;
    {
      const float4* wi = gW1inv + lane;
#pragma unroll
      for (int t = 0; t < 8; ++t) sr_l1_step(hc, wi[t * 64], cur[2 * t], cur[2 * t + 1]);
      sr_l1_step(hc, wi[8 * 64], cr0, cr1);
      sr_l1_step(hc, wi[9 * 64], cr2, 1.0f);
      const int npose = 3 * p.K;
#pragma unroll 1
      for (int u = 0; u < npose; u += 2) {
        const int ka = u / 3, ia = u - 3 * ka, kb = (u + 1) / 3, ib = (u + 1) - 3 * kb;
        const float fa = geom_b[ka * SR_GEOM_STRIDE + 15 + ia];
        const float fb = (u + 1 < npose) ? geom_b[kb * SR_GEOM_STRIDE + 15 + ib] : 0.0f;
        sr_l1_step(hc, wi[(size_t)(10 + (u >> 1)) * 64], fa, fb);
      }
    }

    SrSample smp;
    float4 taps[16];
    float fn[SR_VIEW_SLOTS];
    unsigned ph[SR_VIEW_SLOTS / 2], pl[SR_VIEW_SLOTS / 2];   // the assembled view as 12 pairs of 16-bit pieces
    float X0, X1, X2, d;
    bool any_depth, any_bounds;
    auto issue_view = [&](int k) {
      sr_project_sample(geom_b + k * SR_GEOM_STRIDE, X0, X1, X2, p.h, p.w, p.inv_w, p.inv_h, smp);
      sr_mlp_load_taps(src_b + (size_t)k * N * C, smp, taps);
    };
    float rv0, rv1, rv2, rsd, rdot;
#define SR_SPLIT_VIEW                                                                     \
    _Pragma("unroll") for (int i = 0; i < SR_VIEW_SLOTS / 2; ++i) S::split(fn[2 * i], fn[2 * i + 1], ph[i], pl[i]);

    float cst[SR_PLANE_CHUNK];
#pragma unroll
    for (int q = 0; q < SR_PLANE_CHUNK; ++q) cst[q] = 0.0f;
#pragma unroll 1
    for (int j = j0; j < j1; ++j) {
      d = plane_ptr[j * p.planes.sd];
      {
#pragma clang fp contract(off)
        X0 = d * r0; X1 = d * r1; X2 = d * r2;
      }
      any_depth = false; any_bounds = false;
      f32x16 acc[2][4];

      {  // view 0, not overlapped
        issue_view(0);
        SR_RAY_A(fn, geom_b, 0) SR_RAY_B(fn) SR_RAY_C(fn)
        SR_INTERP2(fn, 0, 0) SR_INTERP2(fn, 0, 1) SR_INTERP2(fn, 1, 0) SR_INTERP2(fn, 1, 1)
        SR_INTERP2(fn, 2, 0) SR_INTERP2(fn, 2, 1) SR_INTERP2(fn, 3, 0) SR_INTERP2(fn, 3, 1)
        SR_DOT(fn)
        SR_SPLIT_VIEW
      }
      // layer 1 (depth-variant part), software-pipelined over views: view k+1 is assembled (fp32) and split beside the
      // 2 x 24 MFMAs of view k
#define SR_SPL_VIEW_BODY(FIRST)                                                                          \
      {                                                                                                  \
        const int kn = min(k + 1, p.K - 1);                                                              \
        const float* g = geom_b + kn * SR_GEOM_STRIDE;                                                   \
        const sr_u4* wk = W1s + (size_t)k * (SR_SPL_VIEW_WORDS / 4);                                    \
        sr_u4 bPh, bPl, bQh, bQl;                                                                       \
        sr_swap_halves_u4(sr_u4{ph[0], ph[1], ph[2], ph[3]}, sr_u4{ph[4], ph[5], ph[6], ph[7]}, bPh, bQh); \
        sr_swap_halves_u4(sr_u4{pl[0], pl[1], pl[2], pl[3]}, sr_u4{pl[4], pl[5], pl[6], pl[7]}, bPl, bQl); \
        sr_u4 mPh, mPl, mQh, mQl;                                                                       \
        sr_swap_halves_u4(sr_u4{ph[8], ph[9], ph[10], ph[11]}, zero4, mPh, mQh);                        \
        sr_swap_halves_u4(sr_u4{pl[8], pl[9], pl[10], pl[11]}, zero4, mPl, mQl);                        \
        issue_view(kn);                                                                                  \
        sr_spl_step<FMT, (FIRST) ? 1 : 0>(acc, hc, wk + lane, 64, bPh, bPl, bQh, bQl);                   \
        SR_RAY_A(fn, g, kn) SR_RAY_B(fn) SR_RAY_C(fn)                                                    \
        SR_SB                                                                                            \
        sr_spl_step<FMT, 0>(acc, hc, wk + 512 + (lane & 31), 32, mPh, mPl, mQh, mQl);                    \
        SR_INTERP2(fn, 0, 0) SR_INTERP2(fn, 0, 1) SR_INTERP2(fn, 1, 0) SR_INTERP2(fn, 1, 1)              \
        SR_INTERP2(fn, 2, 0) SR_INTERP2(fn, 2, 1) SR_INTERP2(fn, 3, 0) SR_INTERP2(fn, 3, 1)              \
        SR_DOT(fn)                                                                                       \
        SR_SPLIT_VIEW                                                                                    \
        SR_SB                                                                                            \
      }
      {
        const int k = 0;
        SR_SPL_VIEW_BODY(true)
      }
#pragma unroll 1
      for (int k = 1; k < p.K; ++k) SR_SPL_VIEW_BODY(false)

      // layer 2: 8 k-steps; step s takes accumulator registers 8 (s & 1) .. + 7 of tile s >> 1 through LeakyReLU and the split
      f32x16 acc2[2][4];
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        sr_u4 bh[2], bl[2];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float a0 = acc[g][s >> 1][8 * (s & 1) + 2 * i], a1 = acc[g][s >> 1][8 * (s & 1) + 2 * i + 1];
            unsigned hi, lo;
            S::split(sr_vmax(a0, p.slope * a0), sr_vmax(a1, p.slope * a1), hi, lo);
            bh[g][i] = hi;
            bl[g][i] = lo;
          }
        const sr_u4* w2 = W2s + (size_t)s * 512 + lane;
        if (s == 0) sr_spl_step<FMT, 2>(acc2, acc2, w2, 64, bh[0], bl[0], bh[1], bl[1]);
        else sr_spl_step<FMT, 0>(acc2, acc2, w2, 64, bh[0], bl[0], bh[1], bl[1]);
      }

      // layer 3 (128 -> 1) on acc2 + b2; w3tab and b2tab in LDS (C layout)
      const float4* w3 = reinterpret_cast<const float4*>(lds + half * 64);
      const float4* b2t = reinterpret_cast<const float4*>(lds + 256 + half * 64);
      sr_f2v oPQ = {0.0f, 0.0f};
      const sr_f2v slope2 = {p.slope, p.slope};
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 wv = w3[m * 4 + q], bv = b2t[m * 4 + q];
          const float wr[4] = {wv.x, wv.y, wv.z, wv.w}, br[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const sr_f2v h2 = sr_f2v{acc2[0][m][4 * q + i], acc2[1][m][4 * q + i]} + sr_f2v{br[i], br[i]};
            const sr_f2v s2 = slope2 * h2;
            oPQ = __builtin_elementwise_fma(sr_f2v{wr[i], wr[i]}, sr_f2v{sr_vmax(h2.x, s2.x), sr_vmax(h2.y, s2.y)}, oPQ);
          }
        }
      float oP = oPQ.x, oQ = oPQ.y;
      oP += __shfl_xor(oP, 32);
      oQ += __shfl_xor(oQ, 32);
      const float cost = (half ? oQ : oP) + lds[128];

      if (p.vec_store) {
#pragma unroll
        for (int q = 0; q < SR_PLANE_CHUNK; ++q) cst[q] = (j - j0 == q) ? cost : cst[q];
      }
      if (active) {
        if (!p.vec_store) p.out.cv[b * p.out.sb + j * p.out.sd + (int64_t)pix * p.out.sp] = cost;
        if (j == p.D - 1 && p.out.mask) p.out.mask[(size_t)b * N + pix] = (uint8_t)(any_depth && any_bounds);
      }
    }
    if (p.vec_store && active) {
      float* row = p.out.cv + b * p.out.sb + (int64_t)pix * p.out.sp + j0;
#pragma unroll
      for (int q = 0; q < SR_PLANE_CHUNK; q += 4) {
        if (j0 + q + 4 <= j1) *reinterpret_cast<float4*>(row + q) = make_float4(cst[q], cst[q + 1], cst[q + 2], cst[q + 3]);
        else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (j0 + q + i < j1) row[q + i] = cst[q + i];
        }
      }
    }
  }
}

// option SR_OPT_MLP_SPLIT: 0 = fp32 MFMA (the product path), 1 = bf16 pieces, 2 = f16 pieces, -1 = unknown (refused).  An
// exported entry point reads it ONCE and hands the value (`split`) to the pack and the sweep it runs: both see one format.

// lowest_cost = planes[argmax_d volume] (cost_volume.py:338-342, 374-378); first maximum wins
__global__ void sr_argmax_planes_kernel(const float* __restrict__ cv, int64_t sb, int64_t sd, int64_t sp,
                                        SrPlanes planes, int h, int w, int D, float* __restrict__ lowest) {
  const int N = h * w;
  const int pix = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (pix >= N) return;
  const int y = pix / w, x = pix - y * w;
  const float* c = cv + b * sb + (int64_t)pix * sp;
  float best = c[0];
  int bj = 0;
  int j = 1;
  for (; j + 8 <= D; j += 8) {  // 8 loads in flight per thread (the launch has few threads: latency-bound otherwise)
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = c[(int64_t)(j + u) * sd];
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (v[u] > best || (v[u] != v[u] && best == best)) { best = v[u]; bj = j + u; }  // NaN = max, like torch.argmax
  }
  for (; j < D; ++j) {
    const float v = c[(int64_t)j * sd];
    if (v > best || (v != v && best == best)) { best = v; bj = j; }
  }
  lowest[(size_t)b * N + pix] = planes.ptr[b * planes.sb + bj * planes.sd + y * planes.sy + x * planes.sx];
}

// ------------------------------------------------------------------ C ABI -------------

extern "C" size_t sr_mlp_volume_workspace_bytes(int B, int K, int C, int h, int w, int hidden) {
  (void)hidden;
  if (B < 0 || K < 0) return 0;
  return sr_volume_workspace_bytes(B, K, C, h, w) + sr_align_up(sr_mlp_packed_floats(K) * sizeof(float), 256) + 256;
}

// The 64 pixels of a wave (sr_mlp_lane_pixel).  Option SR_OPT_MLP_TILE: 0 = auto, 1 = the flattened strip, 2..4 = 2x32, 4x16,
// 8x8 whatever they pad, -1 = unknown (refused).  auto takes the squarest shape whose tile count is at most 1 % above
// ceil(h*w / 64), else the strip: a ragged tile is a whole wave's work for a part of its pixels, and in a scene without
// dead views there is nothing to win it back with (the project's bar for such scenes is 1 %).  The strip is th = 1, tw = 64.
extern "C" int sr_mlp_volume_tile_shape(int h, int w, int* th, int* tw) {
  if (h <= 0 || w <= 0 || !th || !tw) return SR_ERR_INVALID_ARGUMENT;
  const int mode = sr_opt(SR_OPT_MLP_TILE);
  if (mode < 0 || mode > 4) return SR_ERR_INVALID_ARGUMENT;
  *th = 1; *tw = 64;
  if (mode >= 2) { *th = 1 << (mode - 1); *tw = 64 >> (mode - 1); }
  if (mode == 0) {
    const int64_t flat = ((int64_t)h * w + 63) / 64;
    for (int t = 8; t >= 2; t >>= 1) {
      const int64_t tiles = (int64_t)((h + t - 1) / t) * ((w + 64 / t - 1) / (64 / t));
      if (100 * tiles <= 101 * flat) { *th = t; *tw = 64 / t; break; }
    }
  }
  return SR_OK;
}

static float* sr_ws_packed(void* workspace, int B, int K, int C, int h, int w) {
  return (float*)sr_align_up((size_t)workspace + sr_volume_workspace_bytes(B, K, C, h, w), 256);
}

// reserve_cus = n > 0: the persistent grid leaves n CUs to other streams (one workgroup owns a CU's LDS and registers, so
// nothing else starts on a CU of the sweep); the plane chunk is planned for the CUs that remain.  DepthModel asks for it at
// small batch, where the image-prior encoder's chain of small launches on the side stream is the critical path and would be
// parked for the whole sweep (batch 1, graph replay: 5.72 -> 5.48 ms per frame although the sweep itself takes 14 % longer).
// At batch 8 it costs what it gains (25.4-25.6 vs 25.2-25.5 ms; 27.2 vs 26.5 on the keyframe stream), at 960x736 / 96
// planes it loses 2.4 ms of 46: the caller's decision, by batch size.  A reserve that would leave fewer than 8 CUs is ignored.
// src_nhwc = null: cur is planar [B,16,h,w] and the source features are the workspace copy of sr_volume_prepare; else both are
// the caller's channels-last buffers, cur [B, h*w, 16] and src_nhwc [B*K, h*w, 16], read where they lie.
static int sr_mlp_volume_sweep_reserved(int split, const float* cur, const float* src_nhwc, const float* invK_cur,
                                        const float* planes, int64_t ps_b,
                                        int64_t ps_d, int64_t ps_y, int64_t ps_x, float leaky_slope, int B, int K,
                                        int C, int h, int w, int D, float* out_cv, int64_t cv_sb, int64_t cv_sd,
                                        int64_t cv_sp, float* out_lowest, uint8_t* out_mask, int reserve_cus,
                                        void* workspace, size_t workspace_bytes, void* stream_) {
  if (B < 0 || K <= 0 || C <= 0 || h <= 0 || w <= 0 || D <= 0) return SR_ERR_INVALID_ARGUMENT;
  if (B == 0) return SR_OK;
  if (!cur || !invK_cur || !planes || !out_cv || !workspace) return SR_ERR_INVALID_ARGUMENT;
  if (C != 16) return SR_ERR_UNSUPPORTED;
  if (!(leaky_slope > 0.0f && leaky_slope < 1.0f)) return SR_ERR_UNSUPPORTED;
  if (workspace_bytes < sr_mlp_volume_workspace_bytes(B, K, C, h, w, SR_HID)) return SR_ERR_WORKSPACE_TOO_SMALL;
  hipStream_t stream = (hipStream_t)stream_;
  const int N = h * w;

  SrMlpParams p;
  p.cur = cur; p.src_nhwc = src_nhwc ? src_nhwc : sr_ws_src_nhwc(workspace, B, K); p.cur_nhwc = src_nhwc != nullptr;
  p.invK = invK_cur; p.geom = sr_ws_geom(workspace);
  p.packed = sr_ws_packed(workspace, B, K, C, h, w);
  p.planes = {planes, ps_b, ps_d, ps_y, ps_x};
  p.out = {out_cv, cv_sb, cv_sd, cv_sp, out_lowest, out_mask};
  p.B = B; p.K = K; p.h = h; p.w = w; p.D = D;
  int th, tw;
  if (sr_mlp_volume_tile_shape(h, w, &th, &tw)) return SR_ERR_INVALID_ARGUMENT;   // unknown SR_MLP_TILE
  p.th_log2 = __builtin_ctz(th); p.tw_log2 = __builtin_ctz(tw);
  p.tiles_x = th == 1 ? 0 : (w + tw - 1) / tw;
  p.tiles = th == 1 ? (N + 63) / 64 : p.tiles_x * ((h + th - 1) / th);
  p.inv_w = (float)(1.0 / (double)w);
  p.inv_h = (float)(1.0 / (double)h);
  p.slope = leaky_slope;

  // planes per work unit: as many as possible (the hoisted invariant part is paid once per unit) while the
  // units still spread evenly over the 4*CUs persistent waves
  int cus = sr_device_cus();
  if (reserve_cus > 0 && cus - reserve_cus >= 8) cus -= reserve_cus;
  const long waves = 4L * cus;
  double best_cost = 1e30;
  int best = 1;
  for (int c = SR_PLANE_CHUNK; c >= 1; c >>= 1) {
    const long units = (long)B * p.tiles * ((D + c - 1) / c);
    const long rounds = (units + waves - 1) / waves;
    const double cost = (double)rounds * (c * 1192.0 + 168.0);  // MFMAs per unit: c planes + invariant part
    if (cost < best_cost) { best_cost = cost; best = c; }
  }
  p.chunk = best;
  p.chunks = (D + best - 1) / best;
  p.vec_store = (cv_sd == 1) && (p.chunk % 4 == 0) && sr_rows_aligned(out_cv, cv_sb, cv_sp, 15, 4);
  const long nunits = (long)B * p.tiles * p.chunks;
  const int blocks = (int)((nunits + 3) / 4 < cus ? (nunits + 3) / 4 : cus);
  const size_t w3_bytes = SR_LDS_W3_FLOATS * sizeof(float);
  const size_t w1_bytes = (size_t)sr_mlp_steps_var(K) * 1024;
  const size_t w2_bytes = (size_t)SR_MLP_STEPS2 * 1024;
  const size_t lds_max = 160 * 1024;
  if (split < 0) return SR_ERR_INVALID_ARGUMENT;
  if (split) {   // fenced experiment: both weight blocks must fit the LDS (K <= 7); reads cur planar only
    if (p.cur_nhwc) return SR_ERR_UNSUPPORTED;
    const size_t bytes = ((size_t)SR_SPL_TAB + SR_SPL_W2_WORDS + (size_t)K * SR_SPL_VIEW_WORDS) * 4;
    if (bytes > lds_max) return SR_ERR_UNSUPPORTED;
    const void* fn = split == 1 ? (const void*)sr_mlp_volume_split_kernel<1> : (const void*)sr_mlp_volume_split_kernel<2>;
    if (hipError_t e = sr_allow_lds(fn, bytes)) return sr_hip_rc(e);
    if (split == 1) hipLaunchKernelGGL((sr_mlp_volume_split_kernel<1>), dim3(blocks), dim3(256), bytes, stream, p);
    else hipLaunchKernelGGL((sr_mlp_volume_split_kernel<2>), dim3(blocks), dim3(256), bytes, stream, p);
    int rc = sr_hip_rc(hipGetLastError());
    if (rc) return rc;
    if (out_lowest) rc = sr_launch_argmax_planes(out_cv, cv_sb, cv_sd, cv_sp, p.planes, B, h, w, D, out_lowest, stream);
    return rc;
  }
#define SR_MLP_LAUNCH(L1, L2, BYTES)                                                                              \
  {                                                                                                               \
    /* (BYTES grows with K: sr_allow_lds asks again when a later call needs more than the largest grant) */       \
    if (hipError_t e = sr_allow_lds((const void*)sr_mlp_volume_kernel<L1, L2>, (BYTES))) return sr_hip_rc(e);     \
    hipLaunchKernelGGL((sr_mlp_volume_kernel<L1, L2>), dim3(blocks), dim3(256), (BYTES), stream, p);              \
  }
  if (w1_bytes + w2_bytes + w3_bytes <= lds_max) SR_MLP_LAUNCH(true, true, w1_bytes + w2_bytes + w3_bytes)
  else if (w1_bytes + w3_bytes <= lds_max) SR_MLP_LAUNCH(true, false, w1_bytes + w3_bytes)
  else SR_MLP_LAUNCH(false, true, w2_bytes + w3_bytes + 4 * SR_PLANE_CHUNK * 64 * sizeof(float))
#undef SR_MLP_LAUNCH
  int rc = sr_hip_rc(hipGetLastError());
  if (rc) return rc;
  if (out_lowest) rc = sr_launch_argmax_planes(out_cv, cv_sb, cv_sd, cv_sp, p.planes, B, h, w, D, out_lowest, stream);
  return rc;
}

extern "C" int sr_mlp_volume_sweep(const float* cur, const float* invK_cur, const float* planes, int64_t ps_b,
                                   int64_t ps_d, int64_t ps_y, int64_t ps_x, float leaky_slope, int B, int K,
                                   int C, int h, int w, int D, float* out_cv, int64_t cv_sb, int64_t cv_sd,
                                   int64_t cv_sp, float* out_lowest, uint8_t* out_mask, void* workspace,
                                   size_t workspace_bytes, void* stream_) {
  return sr_mlp_volume_sweep_reserved(sr_opt(SR_OPT_MLP_SPLIT), cur, nullptr, invK_cur, planes, ps_b, ps_d, ps_y, ps_x,
                                      leaky_slope, B, K, C, h, w, D, out_cv, cv_sb, cv_sd, cv_sp, out_lowest, out_mask, 0,
                                      workspace, workspace_bytes, stream_);
}

int sr_launch_argmax_planes(const float* cv, int64_t sb, int64_t sd, int64_t sp, SrPlanes planes, int B, int h, int w,
                            int D, float* lowest, hipStream_t stream) {
  hipLaunchKernelGGL(sr_argmax_planes_kernel, dim3((h * w + 63) / 64, B), dim3(64), 0, stream, cv, sb, sd, sp,
                     planes, h, w, D, lowest);
  return sr_hip_rc(hipGetLastError());
}

static int sr_mlp_pack_split(int split, const float* W1, const float* b1, const float* W2, const float* b2,
                             const float* W3, const float* b3, int hidden, int B, int K, int C, int h, int w,
                             void* workspace, size_t workspace_bytes, void* stream_) {
  if (!W1 || !b1 || !W2 || !b2 || !W3 || !b3 || !workspace || K <= 0) return SR_ERR_INVALID_ARGUMENT;
  if (hidden != SR_HID || C != 16) return SR_ERR_UNSUPPORTED;
  if (workspace_bytes < sr_mlp_volume_workspace_bytes(B, K, C, h, w, hidden)) return SR_ERR_WORKSPACE_TOO_SMALL;
  if (split < 0) return SR_ERR_INVALID_ARGUMENT;
  float* packed = sr_ws_packed(workspace, B, K, C, h, w);
  if (split == 1) hipLaunchKernelGGL((sr_mlp_pack_split_kernel<1>), dim3(64), dim3(256), 0, (hipStream_t)stream_, W1, b1, W2, b2, W3, b3, packed, K, C);
  else if (split == 2) hipLaunchKernelGGL((sr_mlp_pack_split_kernel<2>), dim3(64), dim3(256), 0, (hipStream_t)stream_, W1, b1, W2, b2, W3, b3, packed, K, C);
  else hipLaunchKernelGGL(sr_mlp_pack_kernel, dim3(64), dim3(256), 0, (hipStream_t)stream_, W1, b1, W2, b2, W3, b3, packed, K, C);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_mlp_pack_weights(const float* W1, const float* b1, const float* W2, const float* b2,
                                   const float* W3, const float* b3, int hidden, int B, int K, int C, int h, int w,
                                   void* workspace, size_t workspace_bytes, void* stream_) {
  return sr_mlp_pack_split(sr_opt(SR_OPT_MLP_SPLIT), W1, b1, W2, b2, W3, b3, hidden, B, K, C, h, w, workspace, workspace_bytes,
                           stream_);
}

// One body behind sr_mlp_volume_fwd and sr_mlp_volume_fwd_nhwc.  nhwc = false: cur is planar [B,16,h,w] and src [B*K,16,h,w]
// is transposed into the workspace (sr_volume_prepare).  nhwc = true: both already are channels-last (the matching
// encoder's output buffer) -- no transposing copy of either operand, the sweep reads cur [B, h*w, 16] and src
// [B*K, h*w, 16] where the caller keeps them.
static int sr_mlp_volume_run(bool nhwc, const float* cur, const float* src, const float* K_src, const float* T_src_cur,
                             const float* T_cur_src, const float* invK_cur, const float* planes, int64_t ps_b,
                             int64_t ps_d, int64_t ps_y, int64_t ps_x, const float* W1, const float* b1,
                             const float* W2, const float* b2, const float* W3, const float* b3, int hidden,
                             float leaky_slope, int B, int K, int C, int h, int w, int D, float* out_cv,
                             int64_t cv_sb, int64_t cv_sd, int64_t cv_sp, float* out_lowest, uint8_t* out_mask,
                             int reserve_cus, void* workspace, size_t workspace_bytes, void* stream_) {
  if (B < 0 || K <= 0 || C <= 0 || h <= 0 || w <= 0 || D <= 0 || reserve_cus < 0) return SR_ERR_INVALID_ARGUMENT;
  if (B == 0) return SR_OK;
  if (!T_cur_src) return SR_ERR_INVALID_ARGUMENT;
  if (nhwc) {
    if (!cur || !src || !K_src || !T_src_cur || !workspace) return SR_ERR_INVALID_ARGUMENT;
    if (((size_t)cur | (size_t)src) & 15) return SR_ERR_INVALID_ARGUMENT;   // a pixel is read as four 16-byte pieces
  }
  if (hidden != SR_HID || C != 16) return SR_ERR_UNSUPPORTED;
  const int split = sr_opt(SR_OPT_MLP_SPLIT);   // the one read of this call: the pack and the sweep below take the value
  // the split-precision kernel reads cur planar: sr_mlp_volume_fwd serves it
  if (nhwc && split) return split < 0 ? SR_ERR_INVALID_ARGUMENT : SR_ERR_UNSUPPORTED;
  if (workspace_bytes < sr_mlp_volume_workspace_bytes(B, K, C, h, w, hidden)) return SR_ERR_WORKSPACE_TOO_SMALL;
  int rc = nhwc ? sr_launch_geom(K_src, T_src_cur, T_cur_src, sr_ws_geom(workspace), B * K, (hipStream_t)stream_)
                : sr_volume_prepare(src, K_src, T_src_cur, T_cur_src, B, K, C, h, w, workspace, workspace_bytes, stream_);
  if (rc) return rc;
  rc = sr_mlp_pack_split(split, W1, b1, W2, b2, W3, b3, hidden, B, K, C, h, w, workspace, workspace_bytes, stream_);
  if (rc) return rc;
  return sr_mlp_volume_sweep_reserved(split, cur, nhwc ? src : nullptr, invK_cur, planes, ps_b, ps_d, ps_y, ps_x, leaky_slope, B, K,
                                      C, h, w, D, out_cv, cv_sb, cv_sd, cv_sp, out_lowest, out_mask, reserve_cus, workspace,
                                      workspace_bytes, stream_);
}

extern "C" int sr_mlp_volume_fwd(const float* cur, const float* src, const float* K_src, const float* T_src_cur,
                                 const float* T_cur_src, const float* invK_cur, const float* planes, int64_t ps_b,
                                 int64_t ps_d, int64_t ps_y, int64_t ps_x, const float* W1, const float* b1,
                                 const float* W2, const float* b2, const float* W3, const float* b3, int hidden,
                                 float leaky_slope, int B, int K, int C, int h, int w, int D, float* out_cv,
                                 int64_t cv_sb, int64_t cv_sd, int64_t cv_sp, float* out_lowest, uint8_t* out_mask,
                                 int reserve_cus, void* workspace, size_t workspace_bytes, void* stream_) {
  return sr_mlp_volume_run(false, cur, src, K_src, T_src_cur, T_cur_src, invK_cur, planes, ps_b, ps_d, ps_y, ps_x, W1, b1, W2, b2, W3, b3,
                           hidden, leaky_slope, B, K, C, h, w, D, out_cv, cv_sb, cv_sd, cv_sp, out_lowest, out_mask, reserve_cus,
                           workspace, workspace_bytes, stream_);
}

extern "C" int sr_mlp_volume_fwd_nhwc(const float* cur, const float* src, const float* K_src, const float* T_src_cur,
                                      const float* T_cur_src, const float* invK_cur, const float* planes, int64_t ps_b,
                                      int64_t ps_d, int64_t ps_y, int64_t ps_x, const float* W1, const float* b1,
                                      const float* W2, const float* b2, const float* W3, const float* b3, int hidden,
                                      float leaky_slope, int B, int K, int C, int h, int w, int D, float* out_cv,
                                      int64_t cv_sb, int64_t cv_sd, int64_t cv_sp, float* out_lowest, uint8_t* out_mask,
                                      int reserve_cus, void* workspace, size_t workspace_bytes, void* stream_) {
  return sr_mlp_volume_run(true, cur, src, K_src, T_src_cur, T_cur_src, invK_cur, planes, ps_b, ps_d, ps_y, ps_x, W1, b1, W2, b2, W3, b3,
                           hidden, leaky_slope, B, K, C, h, w, D, out_cv, cv_sb, cv_sd, cv_sp, out_lowest, out_mask, reserve_cus,
                           workspace, workspace_bytes, stream_);
}
