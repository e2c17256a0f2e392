// sr_conv16_wgrad.hip -- 16-bit-operand backward pieces of the autocast training path (gfx950; opt-in: SR_AUTOCAST_MFMA16_WGRAD,
// DESIGN.md 3.8a).  The saved activation and the post-activation gradient of a layer whose forward ran on sr_conv16_nhwc_fwd
// are 16-bit values already: the weight gradient multiplies them as they are, with an fp32 accumulator.
//
//   sr_conv16_wgrad_nhwc    dW[co][ci][ky][kx] = sum_{b,y,x} g[b,y,x,co] * in[b, s y + ky - p, s x + kx - p, ci]
//     on v_mfma_f32_32x32x16_{f16,bf16}: M = co, N = ci, K = 16 output pixels per step.  The plan is sr_conv_wgrad_kernel's
//     (sr_conv_bwd.hip): a workgroup owns a 64 x 64 (co, ci) block and a strided share of the (image, output row, 32-pixel
//     segment) items, stages the gradient segment and the k input rows of an item in LDS, wave (co half, ci half) keeps its
//     k*k accumulator tiles over ALL its items and writes them once as a partial [tap][64 co][64 ci] slab; the slabs of a block
//     are added in index order by sr_conv_wgrad_reduce_kernel (no atomics: two runs give the same bits).
//     What is new is the operand layout.  K is pixels and memory is channels-last: lane l of a 32x32x16 MFMA holds
//     A[row l & 31][k = 8 (l >> 5) + j], j = 0..7 -- eight consecutive PIXELS of one channel, the transpose of what a 16-byte
//     load delivers, for both operands.  The rows are staged pixel-major exactly as they lie in memory (one 16-byte chunk =
//     8 channels of a pixel per lane) and the fragments are read with the transposed LDS read ds_read_b64_tr_b16: per 16-lane
//     group a block of 4 pixel rows x 16 channels, lane 4 q + p supplying the address of row q, channels 4 p .. 4 p + 3, lane i
//     receiving channel i of the four rows.  Two reads make a fragment (pixels j = 0..3 and 4..7).  Every lane supplies its
//     own row address, so the input pixels s x + kx - p of a stride-2 layer are just other rows.
//     The transposed read needs EXEC all ones (every read sits in wave-uniform control flow; the tile is padded, nothing is
//     masked), 8-byte aligned lane addresses (row pitches and channel offsets are multiples of 8 bytes) and a 16-byte aligned
//     LDS base.  LDS row pitch: 64 channels are 128 bytes; a 32-lane half reads 4 rows x 64 bytes, and rows 256 bytes apart
//     share banks, so rows are padded to 192 bytes (stride 1: rows q = 0..3 then start at banks 0, 48, 32, 16) and, where the
//     lanes of a block are TWO rows apart (stride-2 input), to 160 bytes (0, 16, 32, 48).  The pad is never read.
//     Everything that must count as zero is STORED as zero: padding taps, pixels past Wo (the K tail of a segment), channels
//     past Cin / Cout inside a 64-block.  Every LDS byte a fragment reads is written for every item, from operand data or as
//     zero -- never uninitialised LDS, never memory outside the operands (0 x NaN is NaN).
//
//   sr_act_bwd_bias16_nhwc  grad_pre = round_to(io, grad * LeakyReLU'(saved output)), d_bias = column sums of the UNROUNDED
//     products: sr_act_bwd_bias_nhwc on 16-bit tensors, 8 channels (16 bytes of a 16-bit tensor) per lane, no casts around it.
#include "sr_buffer.h"
#include "sr_view.h"

namespace {

#define W16_P 32        // output pixels of a segment (two 16-pixel K steps)
#define W16_CT 64       // channels per block side

typedef short w16_s4 __attribute__((ext_vector_type(4)));
typedef short w16_s8 __attribute__((ext_vector_type(8)));

template <int IO> struct W16Fmt;
template <> struct W16Fmt<1> {
  typedef _Float16 e;
  typedef _Float16 e8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ f32x16 mfma(w16_s8 a, w16_s8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(e8, a), __builtin_bit_cast(e8, b), c, 0, 0, 0);
  }
};
template <> struct W16Fmt<2> {
  typedef __bf16 e;
  typedef __bf16 e8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ f32x16 mfma(w16_s8 a, w16_s8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(e8, a), __builtin_bit_cast(e8, b), c, 0, 0, 0);
  }
};

// ds_read_b64_tr_b16 at LDS byte address `p` (8-byte aligned; EXEC must be all ones)
__device__ __forceinline__ w16_s4 w16_tr_read(const unsigned char* p) {
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) w16_s4*)p);
}
// the fragment of 8 pixel rows `pitch` bytes apart starting at `p` (this lane's address in rows 0..3)
__device__ __forceinline__ w16_s8 w16_fragment(const unsigned char* p, int pitch) {
  const w16_s4 lo = w16_tr_read(p), hi = w16_tr_read(p + 4 * pitch);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

struct SrWgrad16Params {
  const uint16_t* x; int64_t x_sb, x_sp;      // input  [B, H, W, Cin]  (channels-last view, strides in elements)
  const uint16_t* g; int64_t g_sb, g_sp;      // dL/dy  [B, Ho, Wo, Cout]
  float* part;                                // [blocks][wgs_per_block][k*k][64 co][64 ci] partial slabs
  int H, W, Cin, Cout, Ho, Wo;
  int ci_blocks, items, wgs_per_block;
};

// The staging loads of the NEXT item are issued into registers before the current item's MFMA loop and stored to LDS after it
// (sr_conv_wgrad_kernel's PIPE form).  Every load is unconditional, from an address inside the operand (the image's first
// pixel where the chunk is dead); a dead chunk is replaced by zero WHERE IT IS STORED (`live` keeps one bit per chunk): a select
// next to the load made the compiler wait for the loads in front of the MFMA loop they are meant to hide behind.
template <int IO, int KS, int ST>
__global__ __launch_bounds__(256) void sr_conv16_wgrad_kernel(const SrWgrad16Params p) {
  typedef W16Fmt<IO> F;
  constexpr int TAPS = KS * KS, PAD = KS / 2;
  constexpr int SPAN = ST * (W16_P - 1) + KS;          // input columns under a segment: 32 (1x1), 34 (3x3), 65 (stride 2)
  constexpr int PITCH_G = 192, PITCH_X = ST == 1 ? 192 : 160;   // bytes per staged pixel row (128 of data; see the head)
  constexpr int G_BYTES = W16_P * PITCH_G;
  constexpr int X_CHUNKS = KS * SPAN * (W16_CT / 8);   // 16-byte chunks of the input rows
  constexpr int XS = (X_CHUNKS + 255) / 256;           // per thread: 1 (1x1), 4 (3x3), 7 (stride 2); the gradient: exactly 1
  __shared__ __attribute__((aligned(16))) unsigned char lds[G_BYTES + KS * SPAN * PITCH_X];
  unsigned char* const gs = lds;                       // [32 px][PITCH_G]
  unsigned char* const xs = lds + G_BYTES;             // [KS][SPAN][PITCH_X]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blk = blockIdx.x / p.wgs_per_block, sub = blockIdx.x - blk * p.wgs_per_block;
  const int cob = blk / p.ci_blocks, cib = blk - cob * p.ci_blocks;
  const int co0 = cob * W16_CT, ci0 = cib * W16_CT;
  const int coh = wave & 1, cih = wave >> 1;           // this wave's 32 x 32 quadrant of the block
  const int segs = (p.Wo + W16_P - 1) / W16_P;

  f32x16 acc[TAPS];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.0f;

  const sr_u4 zero = {0u, 0u, 0u, 0u};
  sr_u4 gq, xq[XS];
  unsigned live = 0u;   // bit 0: the gradient chunk, bit 1 + u: input chunk u
  auto fetch = [&](int item) {
    int it = item;
    const int seg = it % segs; it /= segs;
    const int oy = it % p.Ho;
    const int b = it / p.Ho;
    const int ox0 = seg * W16_P;
    {
      const int px = tid >> 3, q = tid & 7;
      const int ox = ox0 + px, c = co0 + 8 * q;
      const bool ok = ox < p.Wo && c < p.Cout;         // (Cout % 8 == 0: an octet is whole or absent)
      const uint16_t* src = p.g + (int64_t)b * p.g_sb + (ok ? ((int64_t)oy * p.Wo + ox) * p.g_sp + c : (int64_t)0);
      gq = *reinterpret_cast<const sr_u4*>(src);
      live = ok ? 1u : 0u;
    }
#pragma unroll
    for (int u = 0; u < XS; ++u) {
      const int e = tid + 256 * u, q = e & 7, pc = e >> 3;
      const int col = pc % SPAN, ky = pc / SPAN;       // compile-time divisor
      const int iy = ST * oy + ky - PAD, ix = ST * ox0 + col - PAD, c = ci0 + 8 * q;
      const bool ok = ky < KS && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W && c < p.Cin;
      const uint16_t* src = p.x + (int64_t)b * p.x_sb + (ok ? ((int64_t)iy * p.W + ix) * p.x_sp + c : (int64_t)0);
      xq[u] = *reinterpret_cast<const sr_u4*>(src);
      live |= ok ? 2u << u : 0u;
    }
  };
  auto stash = [&]() {
    *reinterpret_cast<sr_u4*>(gs + (tid >> 3) * PITCH_G + 16 * (tid & 7)) = (live & 1u) ? gq : zero;
#pragma unroll
    for (int u = 0; u < XS; ++u) {
      const int e = tid + 256 * u;
      if (e < X_CHUNKS) *reinterpret_cast<sr_u4*>(xs + (e >> 3) * PITCH_X + 16 * (e & 7)) = (live & (2u << u)) ? xq[u] : zero;
    }
  };

  // this lane's place in a transposed read: 16-lane group -> (k half, 16-channel half), lane in group -> (row q, quad pp)
  const int kk = lane >> 5, h16 = (lane >> 4) & 1, qq = (lane >> 2) & 3, pp = lane & 3;
  const unsigned char* const a_base = gs + (8 * kk + qq) * PITCH_G + 2 * (32 * coh + 16 * h16 + 4 * pp);
  const unsigned char* const b_base = xs + ST * (8 * kk + qq) * PITCH_X + 2 * (32 * cih + 16 * h16 + 4 * pp);

  fetch(sub);   // (wgs_per_block <= items: every workgroup has an item)
  for (int item = sub; item < p.items; item += p.wgs_per_block) {
    __syncthreads();   // the previous item's fragments are consumed
    stash();
    __syncthreads();
    if (item + p.wgs_per_block < p.items) fetch(item + p.wgs_per_block);   // in flight under this item's MFMAs
    // K loop: 16 output pixels per MFMA step; lane half kk holds pixels 8 kk .. 8 kk + 7 of the step.  Uniform control flow.
#pragma unroll
    for (int ks = 0; ks < W16_P / 16; ++ks) {
      const w16_s8 a = w16_fragment(a_base + 16 * ks * PITCH_G, PITCH_G);             // A[m = co][k = pixel]
#pragma unroll
      for (int t = 0; t < TAPS; ++t) {
        const int ky = t / KS, kx = t - ky * KS;
        const w16_s8 bq = w16_fragment(b_base + (ky * SPAN + ST * 16 * ks + kx) * PITCH_X, ST * PITCH_X);   // B[k = pixel][n = ci]
        acc[t] = F::mfma(a, bq, acc[t]);
      }
    }
  }
  // flush: acc[t][r] = dW[co0 + 32 coh + (r & 3) + 8 (r >> 2) + 4 kk][ci0 + 32 cih + (lane & 31)][tap t] -> this workgroup's slab
  float* slab = p.part + (size_t)blockIdx.x * TAPS * W16_CT * W16_CT;
  const int i = lane & 31;
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r)
      slab[(t * W16_CT + 32 * coh + (r & 3) + 8 * (r >> 2) + 4 * kk) * W16_CT + 32 * cih + i] = acc[t][r];
}

struct W16Plan { int blocks, per, items, ci_blocks, Ho, Wo; };

// blocks = ceil(Cout / 64) ceil(Cin / 64); items = B Ho ceil(Wo / 32); slabs per block = min(ceil(512 / blocks), items):
// about two workgroups per CU in total, a function of the shape alone (so is the summation order)
W16Plan w16_plan(int B, int H, int W, int Cin, int Cout, int k, int stride) {
  W16Plan pl;
  const int pad = k / 2;
  pl.Ho = (H + 2 * pad - k) / stride + 1;
  pl.Wo = (W + 2 * pad - k) / stride + 1;
  pl.ci_blocks = (Cin + W16_CT - 1) / W16_CT;
  pl.blocks = ((Cout + W16_CT - 1) / W16_CT) * pl.ci_blocks;
  pl.items = B * pl.Ho * ((pl.Wo + W16_P - 1) / W16_P);
  pl.per = (2 * 256 + pl.blocks - 1) / pl.blocks;
  if (pl.per > pl.items) pl.per = pl.items;
  if (pl.per < 1) pl.per = 1;
  return pl;
}

template <int IO>
int w16_launch(const SrWgrad16Params& p, int k, int stride, int grid, hipStream_t stream) {
  if (k == 1) hipLaunchKernelGGL((sr_conv16_wgrad_kernel<IO, 1, 1>), dim3(grid), dim3(256), 0, stream, p);
  else if (stride == 1) hipLaunchKernelGGL((sr_conv16_wgrad_kernel<IO, 3, 1>), dim3(grid), dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((sr_conv16_wgrad_kernel<IO, 3, 2>), dim3(grid), dim3(256), 0, stream, p);
  return sr_hip_rc(hipGetLastError());
}

// ---------------------------------------------------------------------------------------------- elementwise ----

template <int IO>
__device__ __forceinline__ void w16_widen8(sr_u4 v, float (&f)[8]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    f[2 * j] = sr_widen<IO>((unsigned short)(v[j] & 0xffffu));
    f[2 * j + 1] = sr_widen<IO>((unsigned short)(v[j] >> 16));
  }
}

// One lane = 8 channels (an octet) of a pixel.  block = LQ octet lanes x PB pixel lanes (lanes with p0 >= PB idle); G32: the
// gradient is fp32 (two 16-byte loads per octet), else the layer's 16-bit type.  Per-block partial column sums (pixel lanes
// added in lane order) go to partial[block][C]; sr_bias_partial_reduce_kernel adds them in block order.
template <int IO, bool G32>
__global__ __launch_bounds__(256) void sr_act_bwd_bias16_kernel(const void* __restrict__ g_, const sr_u4* __restrict__ y,
                                                               sr_u4* __restrict__ gp, float* __restrict__ partial,
                                                               int64_t pixels, int CO, int LQ, int PB, float slope) {
  __shared__ float red[8][256];
  const int q0 = threadIdx.x % LQ, p0 = threadIdx.x / LQ;
  // uniform trip count (the body holds workgroup barriers): lanes whose octet is past CO in the last round only take part in
  // the barriers
  for (int qb = 0; qb < CO; qb += LQ) {
    const int q = qb + q0;
    const bool live = q < CO;
    float s[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) s[j] = 0.0f;
    if (p0 < PB && live) {
      constexpr int U = 4;   // pixels per trip, their loads issued together
      const int64_t step = (int64_t)gridDim.x * PB;
      for (int64_t px0 = (int64_t)blockIdx.x * PB + p0; px0 < pixels; px0 += step * U) {
        sr_u4 v0[U], v1[U], o[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
          const int64_t px = px0 + k * step;
          const int64_t e = (px < pixels ? px : px0) * CO + q;
          if (G32) {
            v0[k] = reinterpret_cast<const sr_u4*>(g_)[2 * e];
            v1[k] = reinterpret_cast<const sr_u4*>(g_)[2 * e + 1];
          } else {
            v0[k] = reinterpret_cast<const sr_u4*>(g_)[e];
          }
          if (y) o[k] = y[e];
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
          const int64_t px = px0 + k * step;
          if (px >= pixels) continue;
          float v[8];
          if (G32) {
            const sr_f4 lo = __builtin_bit_cast(sr_f4, v0[k]), hi = __builtin_bit_cast(sr_f4, v1[k]);
            v[0] = lo.x; v[1] = lo.y; v[2] = lo.z; v[3] = lo.w;
            v[4] = hi.x; v[5] = hi.y; v[6] = hi.z; v[7] = hi.w;
          } else {
            w16_widen8<IO>(v0[k], v);
          }
          if (y) {
            float yo[8];
            w16_widen8<IO>(o[k], yo);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = yo[j] > 0.0f ? v[j] : v[j] * slope;
          }
          if (gp) {
            sr_u4 t;
#pragma unroll
            for (int j = 0; j < 4; ++j) t[j] = (unsigned)sr_narrow<IO>(v[2 * j]) | ((unsigned)sr_narrow<IO>(v[2 * j + 1]) << 16);
            gp[px * CO + q] = t;
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) s[j] += v[j];   // pixel order: deterministic
        }
      }
    }
    if (partial) {   // uniform
#pragma unroll
      for (int j = 0; j < 8; ++j) red[j][threadIdx.x] = s[j];
      __syncthreads();
      if (p0 == 0 && live) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float t = red[j][q0];
          for (int k = 1; k < PB; ++k) t += red[j][k * LQ + q0];
          partial[(int64_t)blockIdx.x * (8 * CO) + 8 * q + j] = t;
        }
      }
      __syncthreads();
    }
  }
}

#define W16_AB_MAX_BLOCKS 1024
int w16_ab_blocks(int64_t pixels, int C) {
  const int CO = C / 8, LQ = CO < 256 ? CO : 256, PB = 256 / LQ;
  int64_t blocks = (pixels + (int64_t)PB * 16 - 1) / ((int64_t)PB * 16);   // >= 16 pixels per lane
  if (blocks > W16_AB_MAX_BLOCKS) blocks = W16_AB_MAX_BLOCKS;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

}  // namespace

extern "C" int sr_conv16_wgrad_supported(int B, int H, int W, int Cin, int Cout, int k, int stride) {
  if (!sr_conv16_supported(B, H, W, Cin, Cout, k, stride)) return 0;   // forms, Cin % 8, Cout % 8, B > 0, 32-bit pixel counts
  const int pad = k / 2;
  const int64_t Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  if ((int64_t)B * Ho * ((Wo + W16_P - 1) / W16_P) >= ((int64_t)1 << 31)) return 0;   // items are counted in 32 bits
  return 1;
}

// The routing rule of SR_AUTOCAST_MFMA16_WGRAD=1, fitted on profiles/r08_conv16_wgrad.txt (scripts/conv16_wgrad_micro.py; batch 8 and 2,
// fp16 and bf16 agree on every row): 1 for the shape classes where sr_act_bwd_bias16_nhwc + this kernel beat the path the same 16-bit
// tensors took before them (fp32 copies of x, out and g, sr_act_bwd_bias_nhwc + sr_conv_wgrad_nhwc, the cast of the gradient back) by
// more than the spread of repeated identical runs (<= 0.06, 0.12 on the smallest 1x1); a class nobody measured gets 0.
//   3x3 / stride 1: 0.25 - 0.86 x the time on every row -- 64 -> 64 from 9 600 output pixels (0.86 x there, 0.25 x at 614 400),
//       128 -> 128 and 256 -> 128 from 2 400 pixels (0.60 - 0.68 x at batch 2, 0.33 - 0.40 x at batch 8);
//   1x1: 0.68 - 0.79 x for 128 -> 64 from 9 600 pixels, 0.59 - 0.64 x for 256 -> 128 from 2 400;
//   3x3 / stride 2: 0.26 - 0.64 x on every row, Cin 24 .. 256, Cout 96 .. 384, 600 .. 153 600 output pixels.
extern "C" int sr_conv16_wgrad_prefers(int B, int H, int W, int Cin, int Cout, int k, int stride) {
  if (!sr_conv16_wgrad_supported(B, H, W, Cin, Cout, k, stride)) return 0;
  const int64_t M = (int64_t)B * ((H - 1) / stride + 1) * ((W - 1) / stride + 1);   // output pixels
  if (stride == 2) return (Cin >= 24 && Cout >= 96 && M >= 600) ? 1 : 0;
  if (k == 3) {
    if (Cin >= 128 && Cout >= 128) return M >= 2400 ? 1 : 0;
    if (Cin >= 64 && Cout >= 64) return M >= 9600 ? 1 : 0;
    return 0;
  }
  if (Cin >= 256 && Cout >= 128) return M >= 2400 ? 1 : 0;
  if (Cin >= 128 && Cout >= 64) return M >= 9600 ? 1 : 0;
  return 0;
}

extern "C" size_t sr_conv16_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout, int k, int stride) {
  if (!sr_conv16_wgrad_supported(B, H, W, Cin, Cout, k, stride)) return 0;
  const W16Plan pl = w16_plan(B, H, W, Cin, Cout, k, stride);
  return (size_t)pl.blocks * pl.per * k * k * W16_CT * W16_CT * sizeof(float);
}

extern "C" int sr_conv16_wgrad_nhwc(const void* in, int64_t in_batch_stride, int in_pix_stride, const void* grad_out,
                                    int64_t g_batch_stride, int g_pix_stride, float* d_weight, int B, int H, int W, int Cin,
                                    int Cout, int k, int stride, int io_dtype, void* workspace, size_t workspace_bytes,
                                    void* stream_) {
  if (!in || !grad_out || !d_weight || !workspace) return SR_ERR_INVALID_ARGUMENT;
  if (!(io_dtype == 1 || io_dtype == 2)) return SR_ERR_INVALID_ARGUMENT;
  if (!(k == 1 || k == 3) || !(stride == 1 || stride == 2) || (k == 1 && stride != 1)) return SR_ERR_INVALID_ARGUMENT;
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return SR_ERR_INVALID_ARGUMENT;
  if (!sr_conv16_wgrad_supported(B, H, W, Cin, Cout, k, stride)) return SR_ERR_UNSUPPORTED;
  // eight channels = one 16-byte access on both operands
  if (!sr_rows_aligned(in, in_batch_stride, in_pix_stride, 15, 8) || !sr_rows_aligned(grad_out, g_batch_stride, g_pix_stride, 15, 8) ||
      in_pix_stride < Cin || g_pix_stride < Cout || in_batch_stride < 0 || g_batch_stride < 0)
    return SR_ERR_UNSUPPORTED;
  if (!sr_ptr_aligned(workspace, 15) || !sr_ptr_aligned(d_weight, 3) ||
      workspace_bytes < sr_conv16_wgrad_workspace_bytes(B, H, W, Cin, Cout, k, stride))
    return SR_ERR_UNSUPPORTED;
  const W16Plan pl = w16_plan(B, H, W, Cin, Cout, k, stride);
  if ((int64_t)pl.blocks * pl.per >= ((int64_t)1 << 31)) return SR_ERR_UNSUPPORTED;
  SrWgrad16Params p;
  p.x = (const uint16_t*)in; p.x_sb = in_batch_stride; p.x_sp = in_pix_stride;
  p.g = (const uint16_t*)grad_out; p.g_sb = g_batch_stride; p.g_sp = g_pix_stride;
  p.part = (float*)workspace;
  p.H = H; p.W = W; p.Cin = Cin; p.Cout = Cout; p.Ho = pl.Ho; p.Wo = pl.Wo;
  p.ci_blocks = pl.ci_blocks; p.items = pl.items; p.wgs_per_block = pl.per;
  hipStream_t stream = (hipStream_t)stream_;
  const int rc = io_dtype == 1 ? w16_launch<1>(p, k, stride, pl.blocks * pl.per, stream)
                               : w16_launch<2>(p, k, stride, pl.blocks * pl.per, stream);
  if (rc != SR_OK) return rc;
  return sr_wgrad_reduce_launch((const float*)workspace, d_weight, Cout, Cin, k * k, pl.ci_blocks, pl.per, pl.blocks, stream);
}

extern "C" size_t sr_act_bwd_bias16_workspace_bytes(int64_t pixels, int C) {
  if (pixels <= 0 || C <= 0 || C % 8 != 0) return 0;
  return (size_t)w16_ab_blocks(pixels, C) * C * sizeof(float);
}

extern "C" int sr_act_bwd_bias16_nhwc(const void* grad, int grad_dtype, const void* out_saved, void* grad_pre, float* d_bias,
                                      int64_t pixels, int C, float leaky_slope, int io_dtype, void* workspace,
                                      size_t workspace_bytes, void* stream_) {
  if (!(io_dtype == 1 || io_dtype == 2) || !(grad_dtype == 0 || grad_dtype == io_dtype)) return SR_ERR_INVALID_ARGUMENT;
  if (pixels < 0 || C <= 0 || (out_saved && !(leaky_slope >= 0.0f))) return SR_ERR_INVALID_ARGUMENT;
  hipStream_t stream = (hipStream_t)stream_;
  if (pixels == 0) {
    if (d_bias) { const hipError_t e = hipMemsetAsync(d_bias, 0, (size_t)C * sizeof(float), stream); if (e != hipSuccess) return sr_hip_rc(e); }
    return SR_OK;
  }
  if (!grad || (out_saved && !grad_pre)) return SR_ERR_INVALID_ARGUMENT;
  if (!grad_pre && !d_bias) return SR_OK;   // nothing to write
  if (C % 8 != 0 || !sr_ptr_aligned(grad, 15) || !sr_ptr_aligned(out_saved, 15) || !sr_ptr_aligned(grad_pre, 15) ||
      (d_bias && !sr_ptr_aligned(d_bias, 3)))
    return SR_ERR_UNSUPPORTED;
  const int blocks = w16_ab_blocks(pixels, C);
  if (d_bias && (!workspace || !sr_ptr_aligned(workspace, 15) || workspace_bytes < (size_t)blocks * C * sizeof(float)))
    return SR_ERR_WORKSPACE_TOO_SMALL;
  const int CO = C / 8, LQ = CO < 256 ? CO : 256, PB = 256 / LQ;
  float* partial = d_bias ? (float*)workspace : (float*)nullptr;
#define W16_AB_LAUNCH(IOV, G32V)                                                                                        \
  hipLaunchKernelGGL((sr_act_bwd_bias16_kernel<IOV, G32V>), dim3(blocks), dim3(256), 0, stream, grad, (const sr_u4*)out_saved, \
                     (sr_u4*)grad_pre, partial, pixels, CO, LQ, PB, leaky_slope)
  if (io_dtype == 1) { if (grad_dtype == 0) W16_AB_LAUNCH(1, true); else W16_AB_LAUNCH(1, false); }
  else { if (grad_dtype == 0) W16_AB_LAUNCH(2, true); else W16_AB_LAUNCH(2, false); }
#undef W16_AB_LAUNCH
  const int rc = sr_hip_rc(hipGetLastError());
  if (rc != SR_OK || !d_bias) return rc;
  return sr_bias_partial_reduce_launch(partial, blocks, C, d_bias, stream);
}
