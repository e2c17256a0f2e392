// sr_frames.hip -- frame preparation (gfx950): the two-pass fixed-point resize of 8-bit images that Pillow's
// Image.resize does, with the conversion to the model's normalised fp32 planes folded in, and the nearest-neighbour
// gather of 16-bit depth maps with its validity masks.  Rules: include/simplerecon_hip.h, section "frame preparation";
// the tables come from simplerecon_amd/frames.py, tests/frames_oracle.py is the numpy restatement.
//
// Fused colour kernel: one workgroup owns kTH output rows x kTW output columns of one image.  It resamples
// horizontally every input row those output rows tap (a contiguous span of the interleaved input per row), keeps the
// results as uint8 in LDS ([rows][kTW * C], what Pillow's intermediate image holds), then resamples vertically from
// LDS.  The tile's slices of both tables and the 256-entry conversion table sit in LDS next to the rows.
#include "sr_common.h"

namespace {

constexpr int kT = 256;
constexpr int kTW = SR_FRAMES_TILE_W, kTH = SR_FRAMES_TILE_H;
constexpr int kBits = 22;   // Pillow's PRECISION_BITS for 8-bit channels

// (2^21 + sum k v) >> 22 clamped to a byte: the sum wraps as Pillow's 32-bit int does on the machines it runs on
__device__ __forceinline__ uint8_t finish8(uint32_t acc) {
  const int v = (int)acc >> kBits;
  return (uint8_t)min(max(v, 0), 255);
}

// Table entry of output index i: tab[i * (2 + taps) + 0] first tap, [1] tap count, [2..] weights.
struct Geometry {
  int h, w, H, W, xk, yk, flip, lds_rows;
};

template <int C, bool F32>
__global__ __launch_bounds__(kT) void sr_frames_resize_kernel(const uint8_t* __restrict__ in, const int32_t* __restrict__ xtab,
                                                              const int32_t* __restrict__ ytab,
                                                              const float* __restrict__ lut, void* __restrict__ out,
                                                              Geometry g) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  constexpr int kPitch = kTW * C;
  // [x table, field-major: (2 + xk) x kTW int32][conversion table: C x 256 fp32, F32 only][rows: lds_rows x kPitch bytes]
  int32_t* xs = (int32_t*)smem;
  float* ls = (float*)(xs + (2 + g.xk) * kTW);
  uint8_t* rows = (uint8_t*)(ls + (F32 ? C * 256 : 0));

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  const int64_t b = blockIdx.z;
  const int tw = min(kTW, g.W - x0), th = min(kTH, g.H - y0);
  const int xe = 2 + g.xk, ye = 2 + g.yk;

  for (int i = tid; i < xe * tw; i += kT) {
    const int x = i / xe, f = i - x * xe;
    xs[f * kTW + x] = xtab[(int64_t)(x0 + x) * xe + f];
  }
  if (F32)
    for (int i = tid; i < C * 256; i += kT) ls[i] = lut[i];

  // the input rows this tile's output rows tap: [rmin, rmax)
  int rmin = g.h, rmax = 0;
  for (int y = 0; y < th; ++y) {
    const int32_t* e = ytab + (int64_t)(y0 + y) * ye;
    rmin = min(rmin, e[0]);
    rmax = max(rmax, e[0] + e[1]);
  }
  // By contract lds_rows >= rmax - rmin for every tile (frames.rows_needed).  The entry point cannot check that against
  // the table, so the clamp below only keeps a caller's mistake inside the LDS allocation: the output is then undefined.
  const int nrows = min(rmax - rmin, g.lds_rows);
  __syncthreads();

  // horizontal pass: one wave per input row, lanes along the interleaved bytes of the tile's output columns
  const int rowlen = tw * C;
  for (int r = wave; r < nrows; r += kT / 64) {
    const uint8_t* src_row = in + ((b * g.h + rmin + r) * g.w) * C;
    for (int j = lane; j < rowlen; j += 64) {
      const int x = j / C, c = j - x * C;
      const int first = xs[x], n = xs[kTW + x];
      const uint8_t* src = src_row + (int64_t)first * C + c;
      uint32_t acc = 1u << (kBits - 1);
      for (int k = 0; k < n; ++k) acc += (uint32_t)src[k * C] * (uint32_t)xs[(2 + k) * kTW + x];
      rows[r * kPitch + j] = finish8(acc);
    }
  }
  __syncthreads();

  // vertical pass: one wave per output row
  for (int y = wave; y < th; y += kT / 64) {
    const int32_t* e = ytab + (int64_t)(y0 + y) * ye;
    const int first = e[0] - rmin, n = e[1];
    const int64_t yo = y0 + y;
    if (F32) {
      // planes [B,C,H,W]: lanes along x within one channel plane, 256 contiguous bytes per wave store
      for (int c = 0; c < C; ++c) {
        float* dst = (float*)out + ((b * C + c) * g.H + yo) * g.W;
        for (int x = lane; x < tw; x += 64) {
          uint32_t acc = 1u << (kBits - 1);
          for (int k = 0; k < n; ++k) acc += (uint32_t)rows[(first + k) * kPitch + x * C + c] * (uint32_t)e[2 + k];
          const int xo = g.flip ? g.W - 1 - (x0 + x) : x0 + x;
          dst[xo] = ls[c * 256 + finish8(acc)];
        }
      }
    } else {
      uint8_t* dst = (uint8_t*)out + (b * g.H + yo) * g.W * C;
      for (int j = lane; j < rowlen; j += 64) {
        uint32_t acc = 1u << (kBits - 1);
        for (int k = 0; k < n; ++k) acc += (uint32_t)rows[(first + k) * kPitch + j] * (uint32_t)e[2 + k];
        const int x = j / C, c = j - x * C;
        const int xo = g.flip ? g.W - 1 - (x0 + x) : x0 + x;
        dst[(int64_t)xo * C + c] = finish8(acc);
      }
    }
  }
}

// One pass alone, one thread per output byte: the two launches of the path for tiles whose rows do not fit LDS.
// kHorizontal: in [B,h,w,C] -> out [B,h,W,C] uint8.  Otherwise: in [B,h,W,C] -> out [B,H,W,C] uint8 or [B,C,H,W] fp32
// through the conversion table, columns mirrored when flip.
template <int C, bool kHorizontal, bool F32>
__global__ __launch_bounds__(kT) void sr_frames_pass_kernel(const uint8_t* __restrict__ in, const int32_t* __restrict__ tab,
                                                            int taps, const float* __restrict__ lut,
                                                            void* __restrict__ out, int in_rows, int in_cols, int out_rows,
                                                            int out_cols, int flip) {
  // out_cols == in_cols for the vertical pass, out_rows == in_rows for the horizontal one
  const int64_t j = (int64_t)blockIdx.x * kT + threadIdx.x;   // byte within one output row
  if (j >= (int64_t)out_cols * C) return;
  const int x = (int)(j / C), c = (int)(j - (int64_t)x * C);
  const int64_t y = blockIdx.y, b = blockIdx.z;
  const int32_t* e = tab + (int64_t)(kHorizontal ? x : y) * (2 + taps);
  const int first = e[0], n = e[1];
  const uint8_t* src = kHorizontal ? in + ((b * in_rows + y) * in_cols + first) * C + c
                                   : in + ((b * in_rows + first) * in_cols + x) * C + c;
  const int64_t step = kHorizontal ? C : (int64_t)in_cols * C;
  uint32_t acc = 1u << (kBits - 1);
  for (int k = 0; k < n; ++k) acc += (uint32_t)src[k * step] * (uint32_t)e[2 + k];
  const uint8_t v = finish8(acc);
  const int xo = (!kHorizontal && flip) ? out_cols - 1 - x : x;
  if (F32)
    ((float*)out)[((b * C + c) * out_rows + y) * out_cols + xo] = lut[c * 256 + v];
  else
    ((uint8_t*)out)[((b * out_rows + y) * out_cols + xo) * C + c] = v;
}

template <typename T>
__global__ __launch_bounds__(kT) void sr_frames_depth_kernel(const T* __restrict__ in, const int32_t* __restrict__ ysrc,
                                                             const int32_t* __restrict__ xsrc, int h, int w, int H, int W,
                                                             float scale, float min_valid, float max_valid, int flip,
                                                             float* __restrict__ depth, float* __restrict__ mask,
                                                             uint8_t* __restrict__ mask_b) {
#pragma clang fp contract(off)
  const int64_t p = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (p >= (int64_t)H * W) return;
  const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
  const int64_t b = blockIdx.y;
  const float d = (float)in[(b * h + ysrc[y]) * w + xsrc[x]] * scale;
  const bool ok = (d > min_valid) & (d < max_valid);
  const int64_t o = (b * H + y) * W + (flip ? W - 1 - x : x);
  depth[o] = ok ? d : __builtin_nanf("");
  mask[o] = ok ? 1.0f : 0.0f;
  mask_b[o] = ok ? 1 : 0;
}

size_t fused_lds_bytes(int C, int xk, int lds_rows, bool f32) {
  return (size_t)(2 + xk) * kTW * 4 + (f32 ? (size_t)C * 256 * 4 : 0) + (size_t)lds_rows * kTW * C;
}

bool sides_ok(int B, int h, int w, int H, int W, int C) {
  return B >= 1 && B <= SR_FRAMES_MAX_BATCH && C >= 1 && C <= 4 && h >= 1 && w >= 1 && H >= 1 && W >= 1 &&
         h <= SR_FRAMES_MAX_SIDE && w <= SR_FRAMES_MAX_SIDE && H <= SR_FRAMES_MAX_SIDE && W <= SR_FRAMES_MAX_SIDE;
}

template <int C>
int launch_resize(const uint8_t* in, const int32_t* xtab, const int32_t* ytab, const float* lut, void* out, uint8_t* tmp,
                  int B, const Geometry& g, bool f32, hipStream_t st) {
  if (g.lds_rows > 0) {
    const dim3 grid((g.W + kTW - 1) / kTW, (g.H + kTH - 1) / kTH, B);
    const size_t lds = fused_lds_bytes(C, g.xk, g.lds_rows, f32);
    if (f32)
      hipLaunchKernelGGL((sr_frames_resize_kernel<C, true>), grid, dim3(kT), lds, st, in, xtab, ytab, lut, out, g);
    else
      hipLaunchKernelGGL((sr_frames_resize_kernel<C, false>), grid, dim3(kT), lds, st, in, xtab, ytab, lut, out, g);
    return sr_hip_rc(hipGetLastError());
  }
  const dim3 gh((unsigned)(((int64_t)g.W * C + kT - 1) / kT), g.h, B), gv((unsigned)(((int64_t)g.W * C + kT - 1) / kT), g.H, B);
  hipLaunchKernelGGL((sr_frames_pass_kernel<C, true, false>), gh, dim3(kT), 0, st, in, xtab, g.xk, lut, (void*)tmp, g.h, g.w,
                     g.h, g.W, 0);
  if (f32)
    hipLaunchKernelGGL((sr_frames_pass_kernel<C, false, true>), gv, dim3(kT), 0, st, (const uint8_t*)tmp, ytab, g.yk, lut, out,
                       g.h, g.W, g.H, g.W, g.flip);
  else
    hipLaunchKernelGGL((sr_frames_pass_kernel<C, false, false>), gv, dim3(kT), 0, st, (const uint8_t*)tmp, ytab, g.yk, lut,
                       out, g.h, g.W, g.H, g.W, g.flip);
  return sr_hip_rc(hipGetLastError());
}

}  // namespace

extern "C" int sr_frames_resize_fits_lds(int C, int x_taps, int lds_rows, int f32_out) {
  return C >= 1 && C <= 4 && x_taps >= 1 && lds_rows >= 1 &&
         fused_lds_bytes(C, x_taps, lds_rows, f32_out != 0) <= SR_FRAMES_LDS_BYTES;
}

extern "C" int sr_frames_resize(const uint8_t* in, int B, int h, int w, int C, const int32_t* xtab, int x_taps,
                                const int32_t* ytab, int y_taps, int lds_rows, const float* lut, void* out, int f32_out,
                                int H, int W, int flip, uint8_t* tmp, void* stream) {
  if (!in || !xtab || !ytab || !out || x_taps < 1 || y_taps < 1 || lds_rows < 0 || (f32_out && !lut))
    return SR_ERR_INVALID_ARGUMENT;
  if (!sides_ok(B, h, w, H, W, C)) return SR_ERR_UNSUPPORTED;
  if (lds_rows == 0 && !tmp) return SR_ERR_INVALID_ARGUMENT;
  if (lds_rows > 0 && !sr_frames_resize_fits_lds(C, x_taps, lds_rows, f32_out)) return SR_ERR_UNSUPPORTED;
  const Geometry g{h, w, H, W, x_taps, y_taps, flip != 0, lds_rows};
  const hipStream_t st = (hipStream_t)stream;
  switch (C) {
    case 1: return launch_resize<1>(in, xtab, ytab, lut, out, tmp, B, g, f32_out != 0, st);
    case 2: return launch_resize<2>(in, xtab, ytab, lut, out, tmp, B, g, f32_out != 0, st);
    case 3: return launch_resize<3>(in, xtab, ytab, lut, out, tmp, B, g, f32_out != 0, st);
    default: return launch_resize<4>(in, xtab, ytab, lut, out, tmp, B, g, f32_out != 0, st);
  }
}

extern "C" int sr_frames_depth(const void* in, int in_is_int32, int B, int h, int w, const int32_t* ysrc,
                               const int32_t* xsrc, int H, int W, float scale, float min_valid, float max_valid, int flip,
                               float* depth, float* mask, uint8_t* mask_b, void* stream) {
  if (!in || !ysrc || !xsrc || !depth || !mask || !mask_b) return SR_ERR_INVALID_ARGUMENT;
  if (!sides_ok(B, h, w, H, W, 1)) return SR_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(((int64_t)H * W + kT - 1) / kT), B);
  const hipStream_t st = (hipStream_t)stream;
  if (in_is_int32)
    hipLaunchKernelGGL(sr_frames_depth_kernel<int32_t>, grid, dim3(kT), 0, st, (const int32_t*)in, ysrc, xsrc, h, w, H, W,
                       scale, min_valid, max_valid, flip != 0, depth, mask, mask_b);
  else
    hipLaunchKernelGGL(sr_frames_depth_kernel<uint16_t>, grid, dim3(kT), 0, st, (const uint16_t*)in, ysrc, xsrc, h, w, H, W,
                       scale, min_valid, max_valid, flip != 0, depth, mask, mask_b);
  return sr_hip_rc(hipGetLastError());
}
