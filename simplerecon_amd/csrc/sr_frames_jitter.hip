// sr_frames_jitter.hip -- colour jitter of training frames (gfx950): torchvision's ColorJitter on the resized 8-bit
// image, with to_tensor in front and the x-flip and the ImageNet normalisation behind it, in two launches for a whole
// batch.  Rules: include/simplerecon_hip.h, section "frame preparation", part "colour jitter"; the table comes from
// simplerecon_amd/frames.py, tests/jitter_oracle.py is the restatement in torch's CPU operations.
//
// A lane owns 4 consecutive pixels of one row: 12 interleaved input bytes (three aligned words where the width and the
// base allow it), and per colour plane one 16-byte store, so a wave writes 1 KB of a plane row at a time; with flip
// the lane mirrors its own four pixels and writes the mirrored group.  The frame is the block's y index, so the
// frame's operator order is a scalar branch.  Every pixel value is a chain of separately rounded fp32 operations in
// the order of the rule (contraction is off for the whole file), the operations of torch's CPU kernels.
//
// Contrast blends with the mean grey of the image as it stands when the operator runs.  The mean pass applies the
// operators in front of contrast, sums grey in double per workgroup (registers, wave butterfly, LDS) and writes one
// partial per workgroup; the apply pass adds a frame's partials in one fixed tree, so the result is the same bytes on
// every run: no atomics.  A frame without contrast leaves the mean pass at once.
#include "sr_block.h"

#pragma clang fp contract(off)

namespace {

constexpr int kT = 256;
constexpr int kWords = SR_FRAMES_JITTER_PARAM_WORDS;
constexpr int kMaxPartials = SR_FRAMES_JITTER_MAX_PARTIALS;
static_assert(kMaxPartials == 2 * SR_WAVE, "the apply pass adds a frame's partials two per lane");

struct Frame {
  int op[4];                 // operators in the order they run, -1 = empty slot
  float f[3], g[3], hue;     // (factor, 1 - factor) of brightness, contrast, saturation; the hue shift
};

__device__ __forceinline__ Frame load_frame(const int32_t* __restrict__ table, int64_t b) {
  const int32_t* p = table + b * kWords;
  Frame r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r.op[i] = p[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    r.f[i] = __builtin_bit_cast(float, p[4 + 2 * i]);
    r.g[i] = __builtin_bit_cast(float, p[5 + 2 * i]);
  }
  r.hue = __builtin_bit_cast(float, p[10]);
  return r;
}

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }
__device__ __forceinline__ float blend(float a, float b, float f, float g) { return clamp01(f * a + g * b); }
__device__ __forceinline__ float gray(float r, float g, float b) { return 0.2989f * r + 0.587f * g + 0.114f * b; }

// rgb -> hsv, h = (h + shift) mod 1, hsv -> rgb
__device__ __forceinline__ void hue_shift(float& r, float& g, float& b, float shift) {
  const float maxc = fmaxf(fmaxf(r, g), b), minc = fminf(fminf(r, g), b);
  const bool eq = maxc == minc;
  const float cr = maxc - minc;
  const float s = cr / (eq ? 1.0f : maxc);
  const float d = eq ? 1.0f : cr;
  const float rc = (maxc - r) / d, gc = (maxc - g) / d, bc = (maxc - b) / d;
  float h = (maxc == r) ? bc - gc : (maxc == g) ? 2.0f + rc - bc : 4.0f + gc - rc;
  h = h / 6.0f + 1.0f;      // in [5/6, 11/6]
  h = h - floorf(h);        // fmod(h, 1): exact
  h = h + shift;            // in [-1/2, 3/2)
  h = h - floorf(h);        // Python's %: h + 1 for a negative h, rounded, so 1.0 can come out
  const float h6 = h * 6.0f;
  const float fl = floorf(h6);
  const float fr = h6 - fl;
  int i = (int)fl;
  i = i >= 6 ? i - 6 : i;
  const float v = maxc;
  const float p = clamp01(v * (1.0f - s));
  const float q = clamp01(v * (1.0f - s * fr));
  const float t = clamp01(v * (1.0f - s * (1.0f - fr)));
  r = i == 0 ? v : i == 1 ? q : i == 2 ? p : i == 3 ? p : i == 4 ? t : v;
  g = i == 0 ? t : i == 1 ? v : i == 2 ? v : i == 3 ? q : i == 4 ? p : p;
  b = i == 0 ? p : i == 1 ? p : i == 2 ? t : i == 3 ? v : i == 4 ? v : q;
}

// The operators of slots [0, last) on a lane's four pixels.  Contrast (with_mean) blends with `mean`; without it a
// contrast slot is passed over.
__device__ __forceinline__ void run_slots(float (&r)[4], float (&g)[4], float (&b)[4], const Frame& p, int last,
                                          bool with_mean, float mean) {
#pragma unroll 1   // (the slot by selects: a run-time index into the record would move it out of registers)
  for (int s = 0; s < last; ++s) {
    const int op = s == 0 ? p.op[0] : s == 1 ? p.op[1] : s == 2 ? p.op[2] : p.op[3];
    if (op == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {   // the blend with a black image: f x + (1 - f) 0
        r[k] = clamp01(p.f[0] * r[k]);
        g[k] = clamp01(p.f[0] * g[k]);
        b[k] = clamp01(p.f[0] * b[k]);
      }
    } else if (op == 1) {
      if (with_mean) {
        const float gm = p.g[1] * mean;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          r[k] = clamp01(p.f[1] * r[k] + gm);
          g[k] = clamp01(p.f[1] * g[k] + gm);
          b[k] = clamp01(p.f[1] * b[k] + gm);
        }
      }
    } else if (op == 2) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float y = gray(r[k], g[k], b[k]);
        r[k] = blend(r[k], y, p.f[2], p.g[2]);
        g[k] = blend(g[k], y, p.f[2], p.g[2]);
        b[k] = blend(b[k], y, p.f[2], p.g[2]);
      }
    } else if (op == 3) {
#pragma unroll
      for (int k = 0; k < 4; ++k) hue_shift(r[k], g[k], b[k], p.hue);
    }
  }
}

// to_tensor of pixels [x0, x0 + 4) of the row that starts at `row`: float(v) / 255.  Pixels past the row's end are 0.
template <bool WIDE>
__device__ __forceinline__ void load4(const uint8_t* __restrict__ row, int x0, int n, float (&r)[4], float (&g)[4],
                                      float (&b)[4]) {
  uint32_t w[3];
  if (WIDE) {
    const uint32_t* src = (const uint32_t*)(row + (int64_t)x0 * 3);
    w[0] = src[0], w[1] = src[1], w[2] = src[2];
  } else {
    w[0] = w[1] = w[2] = 0;
#pragma unroll
    for (int i = 0; i < 12; ++i)
      if (i < 3 * n) w[i >> 2] |= (uint32_t)row[(int64_t)x0 * 3 + i] << (8 * (i & 3));
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int i = 3 * k;
    r[k] = (float)((w[i >> 2] >> (8 * (i & 3))) & 255u) / 255.0f;
    g[k] = (float)((w[(i + 1) >> 2] >> (8 * ((i + 1) & 3))) & 255u) / 255.0f;
    b[k] = (float)((w[(i + 2) >> 2] >> (8 * ((i + 2) & 3))) & 255u) / 255.0f;
  }
}

// partial [B, G] double: workgroup x of frame b sums the grey of its pixels as they stand in front of contrast
template <bool WIDE>
__global__ __launch_bounds__(kT) void sr_frames_jitter_mean_kernel(const uint8_t* __restrict__ in,
                                                                   const int32_t* __restrict__ table,
                                                                   double* __restrict__ partial, int H, int W, int G) {
  __shared__ double sums[kT / SR_WAVE];
  const int64_t b = blockIdx.y;
  const Frame p = load_frame(table, b);
  const int before = p.op[0] == 1 ? 0 : p.op[1] == 1 ? 1 : p.op[2] == 1 ? 2 : p.op[3] == 1 ? 3 : -1;
  if (before < 0) return;   // the whole workgroup: no contrast in this frame, nothing reads its partials
  const int gpr = (W + 3) >> 2;
  const int groups = gpr * H;   // at most 2^28: the sides are at most SR_FRAMES_MAX_SIDE
  double acc = 0.0;
  for (int i = blockIdx.x * kT + threadIdx.x; i < groups; i += G * kT) {
    const int y = i / gpr, x0 = (i - y * gpr) * 4;
    const int n = min(4, W - x0);
    float r[4], g[4], bl[4];
    load4<WIDE>(in + ((b * H + y) * W) * 3, x0, n, r, g, bl);
    run_slots(r, g, bl, p, before, false, 0.0f);
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k < n) acc += (double)gray(r[k], g[k], bl[k]);
  }
  acc = sr_wave_sum(acc);
  if ((threadIdx.x & (SR_WAVE - 1)) == 0) sums[threadIdx.x / SR_WAVE] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = sums[0];
    for (int w = 1; w < kT / SR_WAVE; ++w) t += sums[w];
    partial[b * G + blockIdx.x] = t;
  }
}

template <bool WIDE>
__global__ __launch_bounds__(kT) void sr_frames_jitter_apply_kernel(const uint8_t* __restrict__ in,
                                                                    const int32_t* __restrict__ table,
                                                                    const double* __restrict__ partial,
                                                                    float* __restrict__ out, int H, int W, int G, int flip,
                                                                    int normalise) {
  const int64_t b = blockIdx.y;
  const Frame p = load_frame(table, b);
  const bool contrast = (p.op[0] == 1) | (p.op[1] == 1) | (p.op[2] == 1) | (p.op[3] == 1);
  const bool with_mean = contrast && partial != nullptr;
  float mean = 0.0f;
  if (with_mean) {
    // every wave adds the frame's G <= 128 partials in the same tree: two per lane, then the butterfly
    const int lane = threadIdx.x & (SR_WAVE - 1);
    const double* q = partial + b * G;
    double t = (lane < G ? q[lane] : 0.0) + (lane + SR_WAVE < G ? q[lane + SR_WAVE] : 0.0);
    t = sr_wave_sum(t);
    mean = (float)(t / ((double)H * (double)W));
  }
  const int gpr = (W + 3) >> 2;
  const int i = blockIdx.x * kT + threadIdx.x;   // below 2^28 + 256: the sides are at most SR_FRAMES_MAX_SIDE
  if (i >= gpr * H) return;
  const int y = i / gpr, x0 = (i - y * gpr) * 4;
  const int n = min(4, W - x0);
  float c[3][4];
  load4<WIDE>(in + ((b * H + y) * W) * 3, x0, n, c[0], c[1], c[2]);
  run_slots(c[0], c[1], c[2], p, 4, with_mean, mean);
  if (normalise) {
    const float mu[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
#pragma unroll
      for (int k = 0; k < 4; ++k) c[ch][k] = (c[ch][k] - mu[ch]) / sd[ch];
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    float* dst = out + ((b * 3 + ch) * H + y) * W;
    if (WIDE) {
      if (flip)
        *(float4*)(dst + (W - 4 - x0)) = make_float4(c[ch][3], c[ch][2], c[ch][1], c[ch][0]);
      else
        *(float4*)(dst + x0) = make_float4(c[ch][0], c[ch][1], c[ch][2], c[ch][3]);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (k < n) dst[flip ? W - 1 - (x0 + k) : x0 + k] = c[ch][k];
    }
  }
}

bool sizes_ok(int B, int H, int W) {
  return B >= 1 && B <= SR_FRAMES_MAX_BATCH && H >= 1 && W >= 1 && H <= SR_FRAMES_MAX_SIDE && W <= SR_FRAMES_MAX_SIDE;
}

int64_t workgroups(int H, int W) { return ((int64_t)((W + 3) >> 2) * H + kT - 1) / kT; }
int partials(int H, int W) { return (int)std::min<int64_t>(workgroups(H, W), kMaxPartials); }

}  // namespace

extern "C" size_t sr_frames_jitter_scratch_bytes(int B, int H, int W) {
  return sizes_ok(B, H, W) ? (size_t)B * partials(H, W) * sizeof(double) : 0;
}

extern "C" int sr_frames_jitter_check_params(const void* params_host, int B) {
  if (!params_host || B < 1) return SR_ERR_INVALID_ARGUMENT;
  const int32_t* p = (const int32_t*)params_host;
  for (int64_t b = 0; b < B; ++b) {
    unsigned seen = 0;
    for (int s = 0; s < 4; ++s) {
      const int op = p[b * kWords + s];
      if (op == -1) continue;
      if (op < 0 || op > 3 || (seen >> op & 1u)) return SR_ERR_INVALID_ARGUMENT;
      seen |= 1u << op;
    }
  }
  return SR_OK;
}

extern "C" int sr_frames_jitter(const uint8_t* in_u8, int B, int H, int W, const void* params, float* out, int flip,
                                int normalise, void* scratch, size_t scratch_bytes, void* stream) {
  if (!in_u8 || !params || !out || ((uintptr_t)params & 3) || ((uintptr_t)out & 3)) return SR_ERR_INVALID_ARGUMENT;
  if (!sizes_ok(B, H, W)) return SR_ERR_UNSUPPORTED;
  if (scratch && ((uintptr_t)scratch & 7)) return SR_ERR_INVALID_ARGUMENT;
  if (scratch && scratch_bytes < sr_frames_jitter_scratch_bytes(B, H, W)) return SR_ERR_WORKSPACE_TOO_SMALL;
  const hipStream_t st = (hipStream_t)stream;
  const int32_t* table = (const int32_t*)params;
  double* partial = (double*)scratch;
  const int G = partials(H, W);
  const bool wide = W % 4 == 0 && ((uintptr_t)in_u8 & 3) == 0 && ((uintptr_t)out & 15) == 0;
  const dim3 grid((unsigned)workgroups(H, W), B);
  if (partial) {
    const dim3 mgrid(G, B);
    if (wide)
      hipLaunchKernelGGL(sr_frames_jitter_mean_kernel<true>, mgrid, dim3(kT), 0, st, in_u8, table, partial, H, W, G);
    else
      hipLaunchKernelGGL(sr_frames_jitter_mean_kernel<false>, mgrid, dim3(kT), 0, st, in_u8, table, partial, H, W, G);
    const int rc = sr_hip_rc(hipGetLastError());
    if (rc != SR_OK) return rc;
  }
  if (wide)
    hipLaunchKernelGGL(sr_frames_jitter_apply_kernel<true>, grid, dim3(kT), 0, st, in_u8, table, (const double*)partial, out,
                       H, W, G, flip != 0, normalise != 0);
  else
    hipLaunchKernelGGL(sr_frames_jitter_apply_kernel<false>, grid, dim3(kT), 0, st, in_u8, table, (const double*)partial, out,
                       H, W, G, flip != 0, normalise != 0);
  return sr_hip_rc(hipGetLastError());
}
