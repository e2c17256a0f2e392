// sr_conv16.hip -- 16-bit MFMA convolutions of the autocast training path (gfx950).  Opt-in (SR_AUTOCAST_MFMA16, DESIGN.md
// 3.8); the reference trains under 16-bit autocast (options.py:100-101, train.py:132), so 16-bit matrix arithmetic with an
// fp32 accumulator is that path's own arithmetic.
//   out = round_to(out_dtype, act(sum + bias + residual))     3x3 / stride 1 | 2 / zero pad 1, or 1x1 / stride 1
// as an implicit GEMM on v_mfma_f32_32x32x16_{f16,bf16}:  D[co][pixel] = sum_k W[co][k] X[k][pixel],  k = (tap, channel).
//   * the WEIGHT is the A operand (rows = output channels), the ACTIVATION the B operand (columns = pixels): the accumulator
//     of lane (pixel l & 31, half l >> 5) then holds channels 8 g + 4 (l >> 5) + i of its pixel in registers 4 g + i -- four
//     consecutive channels per register quad, one 8-byte (16-bit output) or 16-byte (fp32 output) store each;
//   * a k-step is 16 channels of one tap: lane (r, h) reads channels 16 cs + 8 h .. + 7 of its pixel's tap as ONE 16-byte
//     access (Cin % 8 == 0, strides % 8 == 0, 16-byte aligned bases), zero where the tap is outside the image or the channel
//     group is past Cin (Cin = 8, 24, 40: the upper half of the last step) -- nothing is read past a row;
//   * the packed weight is the A fragment image: record (32-channel tile t, tap, k-step cs, lane) = 8 values
//     W[32 t + r][16 cs + 8 h + j][tap], zero outside Cout x Cin; 1 KiB per wave access, shared by every wave through L1 / L2;
//   * no LDS, no barrier, no atomics, no K split: one wave owns MT x 32 pixels x NT x 32 channels and sums taps and channel
//     steps in a fixed order -- two runs give the same bits.
// bias + residual + LeakyReLU run in fp32 on the accumulator; one rounding on the way out.
#include "sr_buffer.h"
#include "sr_view.h"

namespace {

template <int IO> struct C16Fmt;
template <> struct C16Fmt<1> {
  typedef _Float16 e;
  typedef _Float16 e4 __attribute__((ext_vector_type(4)));
  typedef _Float16 e8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ f32x16 mfma(sr_u4 a, sr_u4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(e8, a), __builtin_bit_cast(e8, b), c, 0, 0, 0);
  }
};
template <> struct C16Fmt<2> {
  typedef __bf16 e;
  typedef __bf16 e4 __attribute__((ext_vector_type(4)));
  typedef __bf16 e8 __attribute__((ext_vector_type(8)));
  static __device__ __forceinline__ f32x16 mfma(sr_u4 a, sr_u4 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(e8, a), __builtin_bit_cast(e8, b), c, 0, 0, 0);
  }
};

struct SrConv16Params {
  const uint16_t* in; int64_t in_sb, in_sp;
  const uint16_t* wp;
  const float* bias;
  const uint16_t* res; int64_t res_sb, res_sp;
  void* out; int64_t out_sb, out_sp;
  int H, W, Ho, Wo, Cin, Cout, k, stride;
  int csteps;     // 16-channel k-steps per tap
  int tiles_n;    // 32-channel output tiles
  int64_t M;      // output pixels, B * Ho * Wo
  float slope;
  int out_f32;
};

static inline int c16_csteps(int Cin) { return (Cin + 15) / 16; }
static inline int c16_tiles(int Cout) { return (Cout + 31) / 32; }

// fp32 [Co][Ci][k][k] -> A-fragment records (see the head of the file); one thread per 16-byte record
template <int IO>
__global__ void sr_conv16_pack_kernel(const float* __restrict__ w, sr_u4* __restrict__ wp, int Co, int Ci, int k,
                                      int csteps, int64_t records) {
  typedef typename C16Fmt<IO>::e8 e8;
  const int taps = k * k;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < records; e += (int64_t)gridDim.x * blockDim.x) {
    const int lane = (int)(e & 63);
    int64_t r = e >> 6;
    const int cs = (int)(r % csteps); r /= csteps;
    const int tap = (int)(r % taps);
    const int t = (int)(r / taps);
    const int co = 32 * t + (lane & 31), c0 = 16 * cs + 8 * (lane >> 5);
    e8 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ci = c0 + j;
      const float f = (co < Co && ci < Ci) ? w[((int64_t)co * Ci + ci) * taps + tap] : 0.0f;
      v[j] = (typename C16Fmt<IO>::e)f;   // round to nearest even; fp16 overflow -> inf
    }
    wp[e] = __builtin_bit_cast(sr_u4, v);
  }
}

template <int IO, int MT, int NT, int D>
__global__ __launch_bounds__(256) void sr_conv16_kernel(const SrConv16Params p) {
  typedef C16Fmt<IO> F;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const int tile0 = blockIdx.y * NT;
  const int n_valid = min(NT, p.tiles_n - tile0);   // (tiles past it are computed on a re-read record and dropped)
  const int64_t m0 = ((int64_t)blockIdx.x * 4 + wave) * (32 * MT);
  if (m0 >= p.M) return;   // (no barrier anywhere: a wave without pixels just leaves)
  const int taps = p.k * p.k, pad = p.k >> 1;
  const int HoWo = p.Ho * p.Wo;

  bool pv[MT];
  int iy0[MT], ix0[MT];
  int64_t in_img[MT], px_lin[MT], img[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int64_t pm = m0 + 32 * m + r;
    pv[m] = pm < p.M;
    const int64_t pc = pv[m] ? pm : 0;
    img[m] = pc / HoWo;
    const int rem = (int)(pc - img[m] * HoWo);
    const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
    px_lin[m] = rem;
    iy0[m] = oy * p.stride - pad;
    ix0[m] = ox * p.stride - pad;
    in_img[m] = img[m] * p.in_sb;
  }

  f32x16 acc[MT][NT];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[m][n][i] = 0.0f;

  const sr_u4 zero = {0u, 0u, 0u, 0u};
  const sr_u4* wrec = (const sr_u4*)p.wp + lane;
  // Fragments of k-step (tap, cs): NT weight records, MT activation groups.  Every load is UNCONDITIONAL, from an address
  // clamped into the tensor (a conditional load makes the compiler wait for it at the end of its branch, which empties the
  // ring below); what must read as zero -- a tap outside the image, a channel group past Cin, a pixel past the last one, a
  // request past the last k-step -- is replaced by zero where the fragment is used (`bok`, `live`).  Tiles past the last one
  // re-read it: their results are never stored.
  auto load = [&](int tap, int cs, bool live, sr_u4 (&af)[NT], sr_u4 (&bf)[MT], bool (&bok)[MT]) {
    const int kh = tap / p.k, kw = tap - kh * p.k;
    const int c = 16 * cs + 8 * hh;
    const bool cok = live & (c < p.Cin);
    const int cc = c < p.Cin ? c : 0;
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const int iy = iy0[m] + kh, ix = ix0[m] + kw;
      bok[m] = pv[m] & cok & ((unsigned)iy < (unsigned)p.H) & ((unsigned)ix < (unsigned)p.W);
      const int iyc = min(max(iy, 0), p.H - 1), ixc = min(max(ix, 0), p.W - 1);
      bf[m] = *(const sr_u4*)(p.in + in_img[m] + ((int64_t)iyc * p.W + ixc) * p.in_sp + cc);
    }
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int t = min(tile0 + n, p.tiles_n - 1);
      af[n] = wrec[(((int64_t)t * taps + tap) * p.csteps + cs) * 64];
    }
  };

  // D-deep register ring: the fragments of k-step s + D - 1 are requested before the MFMAs of step s issue, so D - 1 steps of
  // loads are in flight behind the matrix pipe.  Requests past the last step re-read the last one and multiply as 0 x 0.
  sr_u4 a[D][NT], b[D][MT];
  bool bok[D][MT], live[D];
  const int steps = taps * p.csteps;
  int ltap = 0, lcs = 0, ls = 0;   // the next k-step to load
  auto load_next = [&](int d) {
    live[d] = ls < steps;
    load(ltap, lcs, live[d], a[d], b[d], bok[d]);
    ++ls;
    if (++lcs == p.csteps) { lcs = 0; ++ltap; }
    if (ltap == taps) { ltap = taps - 1; lcs = p.csteps - 1; }   // (clamped: stays on the last record)
  };
#pragma unroll
  for (int d = 0; d < D - 1; ++d) load_next(d);
  for (int s0 = 0; s0 < steps; s0 += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
      load_next((d + D - 1) % D);
      sr_u4 af[NT], bf[MT];
#pragma unroll
      for (int n = 0; n < NT; ++n) af[n] = live[d] ? a[d][n] : zero;
#pragma unroll
      for (int m = 0; m < MT; ++m) bf[m] = bok[d][m] ? b[d][m] : zero;
#pragma unroll
      for (int m = 0; m < MT; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[m][n] = F::mfma(af[n], bf[m], acc[m][n]);
    }
  }

  // epilogue: register quad g of tile n = channels 32 (tile0 + n) + 8 g + 4 hh .. + 3 of this lane's pixel
  const float slope = sr_uniform(p.slope);
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    if (!pv[m]) continue;
    const int64_t o_off = img[m] * p.out_sb + px_lin[m] * p.out_sp;
    const int64_t r_off = img[m] * p.res_sb + px_lin[m] * p.res_sp;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      if (n >= n_valid) continue;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int ch = 32 * (tile0 + n) + 8 * g + 4 * hh;
        if (ch >= p.Cout) continue;   // (Cout % 8 == 0: a quad is whole or absent)
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = acc[m][n][4 * g + i];
        if (p.bias) {
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] += p.bias[ch + i];
        }
        if (p.res) {
          const sr_u2 rr = *(const sr_u2*)(p.res + r_off + ch);
          const sr_f4 rf = __builtin_convertvector(__builtin_bit_cast(typename F::e4, rr), sr_f4);
#pragma unroll
          for (int i = 0; i < 4; ++i) v[i] += rf[i];
        }
        sr_activate_group(v, slope);
        const sr_f4 vf = {v[0], v[1], v[2], v[3]};
        if (p.out_f32) {
          *(sr_f4*)((float*)p.out + o_off + ch) = vf;
        } else {
          const typename F::e4 q = __builtin_convertvector(vf, typename F::e4);   // round to nearest even
          *(sr_u2*)((uint16_t*)p.out + o_off + ch) = __builtin_bit_cast(sr_u2, q);
        }
      }
    }
  }
}

template <int IO, int MT, int NT, int D>
int c16_launch(const SrConv16Params& p, hipStream_t stream) {
  const int64_t gx = (p.M + 128 * MT - 1) / (128 * MT);
  const int gy = (p.tiles_n + NT - 1) / NT;
  hipLaunchKernelGGL((sr_conv16_kernel<IO, MT, NT, D>), dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, stream, p);
  return sr_hip_rc(hipGetLastError());
}

// Tile plan: a wave owns MT x 32 pixels x NT x 32 channels.  Bigger tiles read fewer fragment bytes per MFMA (MT + NT loads for
// MT NT MFMAs); smaller ones make more waves.  The biggest plan that still gives every SIMD two waves (the loads of one wave
// hide behind the other's MFMAs), else the plan with the most waves.
template <int IO>
int c16_dispatch(const SrConv16Params& p, hipStream_t stream) {
  const int64_t want = 2 * (int64_t)sr_device_cus();   // workgroups of 4 waves: two waves per SIMD
  const int64_t m128 = (p.M + 127) / 128, m256 = (p.M + 255) / 256;
  const int t = p.tiles_n;
  if (t >= 2 && m256 * ((t + 1) / 2) >= want) return c16_launch<IO, 2, 2, 4>(p, stream);
  if (t >= 2 && m128 * ((t + 1) / 2) >= want) return c16_launch<IO, 1, 2, 4>(p, stream);
  if (t == 1 && m256 >= want) return c16_launch<IO, 2, 1, 4>(p, stream);
  return c16_launch<IO, 1, 1, 4>(p, stream);
}

}  // namespace

extern "C" int sr_conv16_supported(int B, int H, int W, int Cin, int Cout, int k, int stride) {
  if (B <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0) return 0;
  if (!(k == 3 || k == 1) || !(stride == 1 || stride == 2) || (k == 1 && stride != 1)) return 0;
  if (Cin % 8 != 0 || Cout % 8 != 0) return 0;
  const int pad = k / 2;
  const int64_t Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
  if (Ho <= 0 || Wo <= 0 || Ho * Wo >= ((int64_t)1 << 31) || (int64_t)B * Ho * Wo >= ((int64_t)1 << 37)) return 0;
  if ((int64_t)H * W >= ((int64_t)1 << 31)) return 0;
  return 1;
}

// The routing rule of SR_AUTOCAST_MFMA16=1, fitted on profiles/r07_conv16.txt (scripts/conv16_micro.py; batch 8 and 2, fp16 and bf16
// agree on every row): 1 for the shape classes where this kernel beat the path the same 16-bit tensors took before it by more than
// the spread of repeated identical runs; a class nobody measured gets 0.
//   3x3 / stride 2 (before: boundary conversion + the fp32 direct kernel): 0.28 - 0.53 x the time on every row, Cin 24 .. 256,
//       Cout 96 .. 384, 600 .. 153 600 output pixels;
//   3x3 / stride 1 (before: fp32 Winograd F(2x2) with 16-bit I/O): 0.76 - 0.91 x with Cin, Cout >= 128 from 2 400 pixels up;
//       64 -> 64 wins at 153 600 pixels and more (0.73 - 0.88 x) and ties or loses at 38 400 and fewer (0.98 - 1.02 x);
//   1x1 (before: the fp32 pointwise GEMM with 16-bit I/O): 1.05 - 1.08 x on both classes (the kernel alone is faster, the
//       cast + pack of the weight in front of it is not) -> never.
extern "C" int sr_conv16_prefers(int B, int H, int W, int Cin, int Cout, int k, int stride) {
  if (!sr_conv16_supported(B, H, W, Cin, Cout, k, stride) || k != 3) return 0;
  const int64_t M = (int64_t)B * ((H - 1) / stride + 1) * ((W - 1) / stride + 1);   // output pixels
  if (stride == 2) return (Cin >= 24 && Cout >= 96 && M >= 600) ? 1 : 0;
  if (Cin >= 128 && Cout >= 128) return M >= 2400 ? 1 : 0;
  if (Cin >= 64 && Cout >= 64) return M >= 153600 ? 1 : 0;
  return 0;
}

extern "C" size_t sr_conv16_packed_weight_bytes(int Cout, int Cin, int k) {
  if (Cout <= 0 || Cin <= 0 || !(k == 1 || k == 3)) return 0;
  return (size_t)c16_tiles(Cout) * k * k * c16_csteps(Cin) * 64 * 16;
}

extern "C" int sr_conv16_pack_weights(const float* weight, int Cout, int Cin, int k, int dtype, void* packed, void* stream_) {
  if (!weight || !packed || Cout <= 0 || Cin <= 0 || !(k == 1 || k == 3) || !(dtype == 1 || dtype == 2))
    return SR_ERR_INVALID_ARGUMENT;
  if (!sr_ptr_aligned(packed, 15) || !sr_ptr_aligned(weight, 3)) return SR_ERR_UNSUPPORTED;
  const int csteps = c16_csteps(Cin);
  const int64_t records = (int64_t)c16_tiles(Cout) * k * k * csteps * 64;
  const unsigned grid = (unsigned)((records + 255) / 256 < 4096 ? (records + 255) / 256 : 4096);
  hipStream_t stream = (hipStream_t)stream_;
  if (dtype == 1)
    hipLaunchKernelGGL(sr_conv16_pack_kernel<1>, dim3(grid), dim3(256), 0, stream, weight, (sr_u4*)packed, Cout, Cin, k, csteps,
                       records);
  else
    hipLaunchKernelGGL(sr_conv16_pack_kernel<2>, dim3(grid), dim3(256), 0, stream, weight, (sr_u4*)packed, Cout, Cin, k, csteps,
                       records);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_conv16_nhwc_fwd(const void* in, int64_t in_batch_stride, int in_pix_stride, const void* packed_w,
                                  const float* bias, const void* residual, int64_t res_batch_stride, int res_pix_stride,
                                  void* out, int64_t out_batch_stride, int out_pix_stride, int B, int H, int W, int Cin,
                                  int Cout, int k, int stride, float leaky_slope, int io_dtype, int out_dtype, void* stream_) {
  if (!(io_dtype == 1 || io_dtype == 2) || !(out_dtype == 0 || out_dtype == io_dtype)) return SR_ERR_INVALID_ARGUMENT;
  if (!(k == 1 || k == 3) || !(stride == 1 || stride == 2) || (k == 1 && stride != 1)) return SR_ERR_INVALID_ARGUMENT;
  if (B < 0 || H <= 0 || W <= 0 || Cin <= 0 || Cout <= 0 || !(leaky_slope == leaky_slope)) return SR_ERR_INVALID_ARGUMENT;
  if (B == 0) return SR_OK;
  if (!in || !packed_w || !out) return SR_ERR_INVALID_ARGUMENT;
  if (!sr_conv16_supported(B, H, W, Cin, Cout, k, stride)) return SR_ERR_UNSUPPORTED;
  if (leaky_slope < -1.5f) return SR_ERR_UNSUPPORTED;   // (SiLU: an inference-path activation)
  // eight channels = one 16-byte access on every 16-bit operand; fp32 output quads are 16 bytes as well
  if (!sr_rows_aligned(in, in_batch_stride, in_pix_stride, 15, 8) || !sr_rows_aligned(out, out_batch_stride, out_pix_stride, 15, 8) ||
      in_pix_stride < Cin || out_pix_stride < Cout || in_batch_stride < 0 || out_batch_stride < 0 ||
      !sr_ptr_aligned(packed_w, 15) || (bias && !sr_ptr_aligned(bias, 3)))
    return SR_ERR_UNSUPPORTED;
  if (residual && (!sr_rows_aligned(residual, res_batch_stride, res_pix_stride, 15, 8) || res_pix_stride < Cout ||
                   res_batch_stride < 0))
    return SR_ERR_UNSUPPORTED;
  const int pad = k / 2;
  SrConv16Params p;
  p.in = (const uint16_t*)in; p.in_sb = in_batch_stride; p.in_sp = in_pix_stride;
  p.wp = (const uint16_t*)packed_w; p.bias = bias;
  p.res = (const uint16_t*)residual; p.res_sb = residual ? res_batch_stride : 0; p.res_sp = residual ? res_pix_stride : 0;
  p.out = out; p.out_sb = out_batch_stride; p.out_sp = out_pix_stride;
  p.H = H; p.W = W; p.Ho = (H + 2 * pad - k) / stride + 1; p.Wo = (W + 2 * pad - k) / stride + 1;
  p.Cin = Cin; p.Cout = Cout; p.k = k; p.stride = stride;
  p.csteps = c16_csteps(Cin); p.tiles_n = c16_tiles(Cout);
  p.M = (int64_t)B * p.Ho * p.Wo;
  p.slope = leaky_slope; p.out_f32 = out_dtype == 0;
  hipStream_t stream = (hipStream_t)stream_;
  return io_dtype == 1 ? c16_dispatch<1>(p, stream) : c16_dispatch<2>(p, stream);
}
