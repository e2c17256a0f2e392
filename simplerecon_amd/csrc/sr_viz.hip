// sr_viz.hip -- depth visualisation (gfx950): the value range of (masked) fp32 maps, the reference's colour mapping
// (utils/visualization_utils.py colormap_image) and the two "unit" pictures of the training log, normals and the
// de-normalised image, as 8-bit interleaved pixels and / or fp32 planes.  Rules: include/simplerecon_hip.h, section
// "visualisation".  Every pixel value is a chain of separately rounded fp32 operations (the __f*_rn intrinsics: no
// contraction), so the results are the reference's CPU results bit for bit.
//
// One workgroup owns SR_VIZ_CHUNK consecutive pixels of one image.  When every operand is 16-byte aligned (4 bytes for
// 8-bit arrays) and the pixel count is a multiple of 4, a thread moves 4 pixels per access; otherwise one.  Both forms
// compute the same values.
#include "sr_common.h"

namespace {

constexpr int kT = 256;
constexpr int kChunk = SR_VIZ_CHUNK;

// ---- value range ---------------------------------------------------------------------------------------------------
// Floats as unsigned keys in their numeric order (-0 below +0): min / max of keys do not depend on the order of the
// comparisons, which is what makes the range the same bits on every run.
__device__ __forceinline__ uint32_t order_key(float x) {
  const uint32_t u = __float_as_uint(x);
  return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
  return __uint_as_float(k ^ ((k & 0x80000000u) ? 0x80000000u : 0xffffffffu));
}

constexpr uint32_t kAny = 1, kNaN = 2;

struct Range {
  uint32_t lo = 0xffffffffu, hi = 0, flags = 0;
  __device__ __forceinline__ void take(float x, bool selected) {
    if (!selected) return;
    if (x != x) {
      flags |= kAny | kNaN;
      return;
    }
    const uint32_t k = order_key(x);
    lo = min(lo, k);
    hi = max(hi, k);
    flags |= kAny;
  }
  __device__ __forceinline__ void merge(uint32_t l, uint32_t h, uint32_t f) {
    lo = min(lo, l);
    hi = max(hi, h);
    flags |= f;
  }
};

// Range of the whole workgroup, valid in thread 0.
__device__ __forceinline__ Range block_range(Range r) {
  __shared__ uint32_t s[kT / SR_WAVE][3];
#pragma unroll
  for (int o = SR_WAVE / 2; o > 0; o >>= 1)
    r.merge(__shfl_xor(r.lo, o), __shfl_xor(r.hi, o), __shfl_xor(r.flags, o));
  const int wave = threadIdx.x / SR_WAVE;
  if ((threadIdx.x & (SR_WAVE - 1)) == 0) {
    s[wave][0] = r.lo;
    s[wave][1] = r.hi;
    s[wave][2] = r.flags;
  }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < kT / SR_WAVE; ++w) r.merge(s[w][0], s[w][1], s[w][2]);
  return r;
}

template <int MK>
__device__ __forceinline__ bool selected(const void* mask, int64_t i) {
  if (MK == SR_VIZ_MASK_U8) return ((const uint8_t*)mask)[i] != 0;
  if (MK == SR_VIZ_MASK_F32) return ((const float*)mask)[i] != 0.0f;   // (NaN is non-zero, as in Tensor.bool())
  return true;
}

// The float value of the mask at 4 consecutive pixels (8-bit masks: 1 / 0).
template <int MK>
__device__ __forceinline__ void mask4(const void* mask, int64_t i, float (&m)[4]) {
  if (MK == SR_VIZ_MASK_U8) {
    const uint32_t v = *(const uint32_t*)((const uint8_t*)mask + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = ((v >> (8 * j)) & 0xffu) ? 1.0f : 0.0f;
  } else if (MK == SR_VIZ_MASK_F32) {
    const float4 v = *(const float4*)((const float*)mask + i);
    m[0] = v.x, m[1] = v.y, m[2] = v.z, m[3] = v.w;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = 1.0f;
  }
}
template <int MK>
__device__ __forceinline__ float mask1(const void* mask, int64_t i) {
  if (MK == SR_VIZ_MASK_U8) return ((const uint8_t*)mask)[i] ? 1.0f : 0.0f;
  if (MK == SR_VIZ_MASK_F32) return ((const float*)mask)[i];
  return 1.0f;
}

// partial [B, chunks, 4] uint32: key of the minimum, key of the maximum, flags, unused
template <bool VEC, int MK>
__global__ __launch_bounds__(kT) void sr_viz_range_kernel(const float* __restrict__ image, const void* __restrict__ mask,
                                                          int64_t n, uint32_t* __restrict__ partial) {
  const int64_t b = blockIdx.y, p0 = (int64_t)blockIdx.x * kChunk;
  const int64_t base = b * n;
  const int count = (int)min((int64_t)kChunk, n - p0);
  Range r;
  if (VEC) {
    for (int i = threadIdx.x * 4; i < count; i += kT * 4) {
      const float4 v = *(const float4*)(image + base + p0 + i);
      float m[4];
      mask4<MK>(mask, base + p0 + i, m);
      r.take(v.x, m[0] != 0.0f);
      r.take(v.y, m[1] != 0.0f);
      r.take(v.z, m[2] != 0.0f);
      r.take(v.w, m[3] != 0.0f);
    }
  } else {
    for (int i = threadIdx.x; i < count; i += kT) r.take(image[base + p0 + i], selected<MK>(mask, base + p0 + i));
  }
  r = block_range(r);
  if (threadIdx.x == 0) {
    uint32_t* out = partial + (b * gridDim.x + blockIdx.x) * 4;
    out[0] = r.lo, out[1] = r.hi, out[2] = r.flags, out[3] = 0;
  }
}

// One workgroup per result: `per` partials each.  range [results, 2] = (min, max); both NaN when a selected value is NaN
// (torch.min / torch.max) or nothing is selected.
__global__ __launch_bounds__(kT) void sr_viz_range_finish_kernel(const uint32_t* __restrict__ partial, int64_t per,
                                                                 float* __restrict__ range) {
  const uint32_t* p = partial + (int64_t)blockIdx.x * per * 4;
  Range r;
  for (int64_t i = threadIdx.x; i < per; i += kT) r.merge(p[i * 4], p[i * 4 + 1], p[i * 4 + 2]);
  r = block_range(r);
  if (threadIdx.x == 0) {
    const bool ok = r.flags == kAny;
    range[blockIdx.x * 2] = ok ? key_value(r.lo) : __builtin_nanf("");
    range[blockIdx.x * 2 + 1] = ok ? key_value(r.hi) : __builtin_nanf("");
  }
}

// ---- pixels ----------------------------------------------------------------------------------------------------------
// (int) clamp(s, 0, 255) truncated toward zero; NaN gives 0.  Serves the table index and the 8-bit pixel value.
__device__ __forceinline__ int trunc255(float s) { return s >= 0.0f ? (s <= 255.0f ? (int)s : 255) : 0; }
__device__ __forceinline__ uint32_t pixel8(float v) { return (uint32_t)trunc255(__fmul_rn(v, 255.0f)); }

// 4 pixels x 3 channels, c[channel][pixel], as 12 interleaved bytes (3 aligned words)
__device__ __forceinline__ void store_rgb4(uint8_t* out, const float (&c)[3][4]) {
  uint32_t q[12];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) q[j * 3 + ch] = pixel8(c[ch][j]);
  uint32_t* w = (uint32_t*)out;
#pragma unroll
  for (int k = 0; k < 3; ++k) w[k] = q[4 * k] | (q[4 * k + 1] << 8) | (q[4 * k + 2] << 16) | (q[4 * k + 3] << 24);
}

struct ColormapArgs {
  const float* image;
  const void* mask;
  const float* lut;
  const float *vmin_dev, *vmax_dev;
  int64_t vmin_stride, vmax_stride, n;
  float vmin, vmax, invalid[3];
  float* out_f32;
  uint8_t* out_u8;
};

template <int MK>
__device__ __forceinline__ void colormap_pixel(const float* lut, float x, float vmin, float d, float m,
                                               const float (&invalid)[3], float (&c)[3]) {
  const int i = trunc255(__fmul_rn(__fdiv_rn(__fsub_rn(x, vmin), d), 255.0f));
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    c[ch] = lut[i * 3 + ch];
    if (MK != SR_VIZ_MASK_NONE)
      c[ch] = __fadd_rn(__fmul_rn(c[ch], m), __fmul_rn(invalid[ch], __fsub_rn(1.0f, m)));
  }
}

template <bool VEC, int MK>
__global__ __launch_bounds__(kT) void sr_viz_colormap_kernel(ColormapArgs a) {
  __shared__ float lut[256 * 3];
  for (int i = threadIdx.x; i < 256 * 3; i += kT) lut[i] = a.lut[i];
  const int64_t b = blockIdx.y, p0 = (int64_t)blockIdx.x * kChunk;
  const int64_t base = b * a.n;
  const int count = (int)min((int64_t)kChunk, a.n - p0);
  const float vmin = a.vmin_dev ? a.vmin_dev[b * a.vmin_stride] : a.vmin;
  const float vmax = a.vmax_dev ? a.vmax_dev[b * a.vmax_stride] : a.vmax;
  const float d = __fsub_rn(vmax, vmin);
  const float invalid[3] = {a.invalid[0], a.invalid[1], a.invalid[2]};
  __syncthreads();
  if (VEC) {
    for (int i = threadIdx.x * 4; i < count; i += kT * 4) {
      const int64_t p = p0 + i;
      const float4 v = *(const float4*)(a.image + base + p);
      const float x[4] = {v.x, v.y, v.z, v.w};
      float m[4], c[3][4];
      mask4<MK>(a.mask, base + p, m);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float cj[3];
        colormap_pixel<MK>(lut, x[j], vmin, d, m[j], invalid, cj);
        c[0][j] = cj[0], c[1][j] = cj[1], c[2][j] = cj[2];
      }
      if (a.out_f32) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
          *(float4*)(a.out_f32 + (b * 3 + ch) * a.n + p) = make_float4(c[ch][0], c[ch][1], c[ch][2], c[ch][3]);
      }
      if (a.out_u8) store_rgb4(a.out_u8 + (base + p) * 3, c);
    }
  } else {
    for (int i = threadIdx.x; i < count; i += kT) {
      const int64_t p = p0 + i;
      float c[3];
      colormap_pixel<MK>(lut, a.image[base + p], vmin, d, mask1<MK>(a.mask, base + p), invalid, c);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        if (a.out_f32) a.out_f32[(b * 3 + ch) * a.n + p] = c[ch];
        if (a.out_u8) a.out_u8[(base + p) * 3 + ch] = (uint8_t)pixel8(c[ch]);
      }
    }
  }
}

// normals: nan_to_num(0.5 * (1 + n)) (NaN -> 0, +-inf -> +-FLT_MAX); colour: (x - mean_c) / std_c
template <int MODE>
__device__ __forceinline__ float unit_value(float x, int ch) {
  if (MODE == SR_VIZ_UNIT_NORMALS) {
    const float v = __fmul_rn(0.5f, __fadd_rn(1.0f, x));
    const float big = 3.40282346638528859812e+38f;
    return v != v ? 0.0f : fminf(fmaxf(v, -big), big);
  }
  // the reference's constants (utils/generic_utils.py reverse_imagenet_normalize), rounded double -> fp32 as torch does
  const float mean[3] = {(float)-2.11790393, (float)-2.03571429, (float)-1.80444444};
  const float stdv[3] = {(float)4.36681223, (float)4.46428571, (float)4.44444444};
  return __fdiv_rn(__fsub_rn(x, mean[ch]), stdv[ch]);
}

template <bool VEC, int MODE>
__global__ __launch_bounds__(kT) void sr_viz_unit_kernel(const float* __restrict__ in, int64_t n,
                                                         float* __restrict__ out_f32, uint8_t* __restrict__ out_u8) {
  const int64_t b = blockIdx.y, p0 = (int64_t)blockIdx.x * kChunk;
  const int count = (int)min((int64_t)kChunk, n - p0);
  if (VEC) {
    for (int i = threadIdx.x * 4; i < count; i += kT * 4) {
      const int64_t p = p0 + i;
      float c[3][4];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float4 v = *(const float4*)(in + (b * 3 + ch) * n + p);
        c[ch][0] = unit_value<MODE>(v.x, ch), c[ch][1] = unit_value<MODE>(v.y, ch);
        c[ch][2] = unit_value<MODE>(v.z, ch), c[ch][3] = unit_value<MODE>(v.w, ch);
        if (out_f32) *(float4*)(out_f32 + (b * 3 + ch) * n + p) = make_float4(c[ch][0], c[ch][1], c[ch][2], c[ch][3]);
      }
      if (out_u8) store_rgb4(out_u8 + (b * n + p) * 3, c);
    }
  } else {
    for (int i = threadIdx.x; i < count; i += kT) {
      const int64_t p = p0 + i;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const float v = unit_value<MODE>(in[(b * 3 + ch) * n + p], ch);
        if (out_f32) out_f32[(b * 3 + ch) * n + p] = v;
        if (out_u8) out_u8[(b * n + p) * 3 + ch] = (uint8_t)pixel8(v);
      }
    }
  }
}

bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

bool shape_ok(int B, int64_t n) { return B >= 1 && B <= SR_VIZ_MAX_BATCH && n >= 1 && n <= SR_VIZ_MAX_PIXELS; }

int64_t chunks(int64_t n) { return (n + kChunk - 1) / kChunk; }

bool mask_ok(const void* mask, int mask_kind) {
  if (mask_kind == SR_VIZ_MASK_NONE) return true;
  return mask && (mask_kind == SR_VIZ_MASK_U8 || mask_kind == SR_VIZ_MASK_F32);
}

bool mask_aligned(const void* mask, int mask_kind) {
  return mask_kind == SR_VIZ_MASK_NONE || aligned(mask, mask_kind == SR_VIZ_MASK_U8 ? 4 : 16);
}

// f.template operator()<VEC, MK>() for the run-time (vec, mask_kind)
template <typename F>
void dispatch(bool vec, int mask_kind, F&& f) {
  if (vec) {
    if (mask_kind == SR_VIZ_MASK_U8) f.template operator()<true, SR_VIZ_MASK_U8>();
    else if (mask_kind == SR_VIZ_MASK_F32) f.template operator()<true, SR_VIZ_MASK_F32>();
    else f.template operator()<true, SR_VIZ_MASK_NONE>();
  } else {
    if (mask_kind == SR_VIZ_MASK_U8) f.template operator()<false, SR_VIZ_MASK_U8>();
    else if (mask_kind == SR_VIZ_MASK_F32) f.template operator()<false, SR_VIZ_MASK_F32>();
    else f.template operator()<false, SR_VIZ_MASK_NONE>();
  }
}

struct RangeLaunch {
  const float* image;
  const void* mask;
  int64_t n;
  uint32_t* partial;
  dim3 grid;
  hipStream_t st;
  template <bool VEC, int MK>
  void operator()() const {
    hipLaunchKernelGGL((sr_viz_range_kernel<VEC, MK>), grid, dim3(kT), 0, st, image, mask, n, partial);
  }
};

struct ColormapLaunch {
  ColormapArgs a;
  dim3 grid;
  hipStream_t st;
  template <bool VEC, int MK>
  void operator()() const {
    hipLaunchKernelGGL((sr_viz_colormap_kernel<VEC, MK>), grid, dim3(kT), 0, st, a);
  }
};

}  // namespace

extern "C" size_t sr_viz_range_workspace_bytes(int B, int64_t n) {
  return shape_ok(B, n) ? (size_t)B * (size_t)chunks(n) * 4 * sizeof(uint32_t) : 0;
}

extern "C" int sr_viz_range(const float* image, const void* mask, int mask_kind, int B, int64_t n, int pooled,
                            float* range, void* workspace, size_t workspace_bytes, void* stream) {
  if (!image || !range || !workspace || !mask_ok(mask, mask_kind)) return SR_ERR_INVALID_ARGUMENT;
  if (!shape_ok(B, n)) return SR_ERR_UNSUPPORTED;
  if (!aligned(workspace, 4)) return SR_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < sr_viz_range_workspace_bytes(B, n)) return SR_ERR_WORKSPACE_TOO_SMALL;
  const hipStream_t st = (hipStream_t)stream;
  const int64_t per = chunks(n);
  const bool vec = n % 4 == 0 && aligned(image, 16) && mask_aligned(mask, mask_kind);
  dispatch(vec, mask_kind, RangeLaunch{image, mask, n, (uint32_t*)workspace, dim3((unsigned)per, B), st});
  hipLaunchKernelGGL(sr_viz_range_finish_kernel, dim3(pooled ? 1 : B), dim3(kT), 0, st, (const uint32_t*)workspace,
                     pooled ? per * B : per, range);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_viz_colormap(const float* image, const void* mask, int mask_kind, int B, int64_t n, const float* lut,
                               const float* vmin_dev, int64_t vmin_stride, const float* vmax_dev, int64_t vmax_stride,
                               float vmin, float vmax, float invalid_r, float invalid_g, float invalid_b,
                               float* out_f32, uint8_t* out_u8, void* stream) {
  if (!image || !lut || (!out_f32 && !out_u8) || !mask_ok(mask, mask_kind) || vmin_stride < 0 || vmax_stride < 0)
    return SR_ERR_INVALID_ARGUMENT;
  if (!shape_ok(B, n)) return SR_ERR_UNSUPPORTED;
  const bool vec = n % 4 == 0 && aligned(image, 16) && mask_aligned(mask, mask_kind) && aligned(out_f32, 16) &&
                   aligned(out_u8, 4);
  const ColormapArgs a{image, mask, lut, vmin_dev, vmax_dev, vmin_stride, vmax_stride, n, vmin, vmax,
                       {invalid_r, invalid_g, invalid_b}, out_f32, out_u8};
  dispatch(vec, mask_kind, ColormapLaunch{a, dim3((unsigned)chunks(n), B), (hipStream_t)stream});
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_viz_unit(const float* in, int B, int64_t n, int mode, float* out_f32, uint8_t* out_u8, void* stream) {
  if (!in || (!out_f32 && !out_u8) || (mode != SR_VIZ_UNIT_NORMALS && mode != SR_VIZ_UNIT_COLOR))
    return SR_ERR_INVALID_ARGUMENT;
  if (!shape_ok(B, n)) return SR_ERR_UNSUPPORTED;
  const bool vec = n % 4 == 0 && aligned(in, 16) && aligned(out_f32, 16) && aligned(out_u8, 4);
  const dim3 grid((unsigned)chunks(n), B);
  const hipStream_t st = (hipStream_t)stream;
#define SR_VIZ_UNIT_LAUNCH(V, M) hipLaunchKernelGGL((sr_viz_unit_kernel<V, M>), grid, dim3(kT), 0, st, in, n, out_f32, out_u8)
  if (mode == SR_VIZ_UNIT_NORMALS) {
    if (vec) SR_VIZ_UNIT_LAUNCH(true, SR_VIZ_UNIT_NORMALS);
    else SR_VIZ_UNIT_LAUNCH(false, SR_VIZ_UNIT_NORMALS);
  } else {
    if (vec) SR_VIZ_UNIT_LAUNCH(true, SR_VIZ_UNIT_COLOR);
    else SR_VIZ_UNIT_LAUNCH(false, SR_VIZ_UNIT_COLOR);
  }
#undef SR_VIZ_UNIT_LAUNCH
  return sr_hip_rc(hipGetLastError());
}
