// sr_losses.hip -- the training objective of the reference (experiment_modules/depth_model.py:409-500 with losses.py
// and utils/geometry_utils.py:92-133), forward and backward.  gfx950 only.
//
// The rules, including the reference's quirks and the three kornia filters it relies on, are stated in
// include/simplerecon_hip.h, section "training losses"; tests/loss_oracle.py restates them in fp64 torch.
//   normals      : blur -> normals from the blurred map; backward in gather form (per pixel: the adjoint of the
//                  normalised cross product, then of the Sobel taps, then of the blur), three gathers, no atomics.
//   grad loss    : one launch per pyramid level builds gt and pred together; one launch takes the masked |dpred - dgt|
//                  of all four levels; the adjoint runs from level 3 down, each level gathering its own Sobel adjoint
//                  and the blur-pool adjoint of the level below it.
//   multi-view   : a thread per (b, pixel) loops over the K sources; its gradient is written once.
//   depth terms  : a thread per gt pixel reads the coarse scales by nearest index; the coarse-scale gradients are
//                  gathered from the fine pixels that read them.
// Every loss ends in per-block partials written in a fixed order and one single-workgroup finalize that sums them in
// fp64 and writes the loss scalars (and the counts / means the backward needs) to device memory: no float atomics, no
// host synchronisation, and two runs give the same bits.
#include "sr_common.h"
#include "sr_block.h"

#pragma clang fp contract(off)

namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / SR_WAVE;
constexpr int kMaxFields = 32;
constexpr float kNormEps = 1e-12f;

enum { kFinNormals = 0, kFinGrad = 1, kFinMV = 2, kFinDepth = 3 };
constexpr int kNormalsFields = 2;   // sum, count
constexpr int kGradFields = 8;      // (sum, count) per level
constexpr int kDepthFields = 11;    // ms0..ms3, count, abs, inv, inv count, log l1, sum d, sum d^2
constexpr int kMVFields = 2 * SR_LOSS_MAX_SOURCES;   // (sum, count) per source

// Every thread of the block calls this with its NF values (zero for idle threads); the block's sums land in
// partials[block * NF + f], each in the same order on every run.
template <int NF>
__device__ __forceinline__ void store_partials(const float (&v)[NF], float* __restrict__ partials, int64_t block) {
  __shared__ float red[kWaves][NF];
  const int lane = threadIdx.x & (SR_WAVE - 1), wv = threadIdx.x / SR_WAVE;
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    const float s = sr_wave_sum(v[f]);
    if (lane == 0) red[wv][f] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < NF) {
    float s = red[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) s += red[k][threadIdx.x];
    partials[block * NF + threadIdx.x] = s;
  }
}

__device__ __forceinline__ float sgnf(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : (x == 0.0f ? 0.0f : x)); }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int reflecti(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }
// max(x, eps) that keeps a NaN (torch's clamp_min)
__device__ __forceinline__ float clamp_min_nan(float x, float lo) { return x < lo ? lo : x; }

// Sobel taps, normalised by 8: gx = correlation with SX, gy with its transpose.  Zero taps are multiplied like the others
// so that a non-finite value anywhere in the 3x3 window makes the component non-finite (as ATen's conv does).
__constant__ float kSX[3][3] = {{-0.125f, 0.0f, 0.125f}, {-0.25f, 0.0f, 0.25f}, {-0.125f, 0.0f, 0.125f}};
__constant__ float kSY[3][3] = {{-0.125f, -0.25f, -0.125f}, {0.0f, 0.0f, 0.0f}, {0.125f, 0.25f, 0.125f}};
// blur_pool2d(x, 3): [1,2,1]^T [1,2,1] / 16
__constant__ float kBP[3] = {1.0f, 2.0f, 1.0f};

// ------------------------------------------------------------------------------------------ finalize ---------------
struct FinParams {
  const float* partials;
  int64_t nblocks;
  int nf;       // fields reduced
  int stride;   // floats per block in `partials`
  int mode;
  int K;          // multi-view: number of sources
  int present;    // depth terms: bit i = scale i present
  float lambda;   // depth terms: si lambda
  float* out;
};

__global__ __launch_bounds__(kT) void sr_loss_finalize_kernel(FinParams p) {
  __shared__ double red[kWaves];
  __shared__ double sums[kMaxFields];
  const int lane = threadIdx.x & (SR_WAVE - 1), wv = threadIdx.x / SR_WAVE;
  for (int f = 0; f < p.nf; ++f) {
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < p.nblocks; i += kT) s += (double)p.partials[i * p.stride + f];
    s = sr_wave_sum(s);
    if (lane == 0) red[wv] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = red[0];
      for (int k = 1; k < kWaves; ++k) t += red[k];
      sums[f] = t;
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  float* o = p.out;
  if (p.mode == kFinNormals) {
    o[0] = (float)(sums[0] / sums[1]);
    o[1] = (float)sums[1];
  } else if (p.mode == kFinGrad) {
    float loss = 0.0f;
    for (int l = 0; l < 4; ++l) {
      loss += (float)(sums[2 * l] / sums[2 * l + 1]);
      o[1 + l] = (float)sums[2 * l + 1];
    }
    o[0] = loss;
  } else if (p.mode == kFinMV) {
    float loss = 0.0f;
    for (int k = 0; k < p.K; ++k) {
      const float m = (float)(sums[2 * k] / sums[2 * k + 1]);   // empty: 0/0 = NaN, as the reference's nanmean
      loss += m;
      o[1 + k] = (float)sums[2 * k + 1];
      o[1 + p.K + k] = m;
    }
    o[0] = loss / (float)p.K;
  } else {
    const double n = sums[4], ni = sums[7];
    float ms = 0.0f;
    for (int i = 0; i < 4; ++i)
      if (p.present >> i & 1) ms += (float)(sums[i] / n) / (float)(1 << i);
    const double md = sums[9] / n, md2 = sums[10] / n;
    o[0] = ms;
    o[1] = (float)(sums[5] / n);
    o[2] = (float)(sums[6] / ni);
    o[3] = (float)(sums[8] / n);
    o[4] = (float)sqrt(md2 - (double)p.lambda * md * md);
    o[5] = (float)n;
    o[6] = (float)ni;
    o[7] = (float)md;
  }
}

int finalize(const float* partials, int64_t nblocks, int nf, int stride, int mode, int K, int present, float lambda,
             float* out, hipStream_t st) {
  FinParams P{partials, nblocks, nf, stride, mode, K, present, lambda, out};
  hipLaunchKernelGGL(sr_loss_finalize_kernel, dim3(1), dim3(kT), 0, st, P);
  return sr_hip_rc(hipGetLastError());
}

unsigned blocks_for(int64_t n) { return (unsigned)((n + kT - 1) / kT); }

// --------------------------------------------------------------------------------------------- normals --------------
struct NormParams {
  const float* depth;    // [B,h,w]
  const float* invK;     // [B,4,4]
  float* s;              // blurred depth [B,h,w]
  float* normals;        // [B,3,h,w]
  const float* gn;       // grad of normals [B,3,h,w]
  float* dG;             // [B,6,h,w]: d gx (3), d gy (3)
  float* ds;             // [B,h,w]
  float* gdepth;         // [B,h,w]
  float g[5];            // gaussian taps
  int h, w;
};

__global__ __launch_bounds__(kT) void sr_normals_blur_kernel(NormParams p) {
  const int hw = p.h * p.w;
  const int pix = blockIdx.x * kT + threadIdx.x;
  if (pix >= hw) return;
  const int64_t base = (int64_t)blockIdx.y * hw;
  const int y = pix / p.w, x = pix - y * p.w;
  float acc = 0.0f;
#pragma unroll
  for (int ty = 0; ty < 5; ++ty) {
    const int yy = reflecti(y + ty - 2, p.h);
#pragma unroll
    for (int tx = 0; tx < 5; ++tx) {
      const int xx = reflecti(x + tx - 2, p.w);
      acc += (p.g[ty] * p.g[tx]) * p.depth[base + yy * p.w + xx];
    }
  }
  p.s[base + pix] = acc;
}

// ray of pixel (x, y): invK[:3,:3] (x + 0.5, y + 0.5, 1)
__device__ __forceinline__ void ray(const float* __restrict__ iK, int x, int y, float r[3]) {
  const float px = (float)x + 0.5f, py = (float)y + 0.5f;
#pragma unroll
  for (int c = 0; c < 3; ++c) r[c] = iK[c * 4 + 0] * px + iK[c * 4 + 1] * py + iK[c * 4 + 2];
}

// Sobel of the back-projected blurred map at (x, y), replicate borders
__device__ __forceinline__ void point_grads(const float* __restrict__ s, const float* __restrict__ iK, int y, int x, int h,
                                            int w, float gx[3], float gy[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) gx[c] = gy[c] = 0.0f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int yy = clampi(y + i - 1, 0, h - 1);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int xx = clampi(x + j - 1, 0, w - 1);
      float r[3];
      ray(iK, xx, yy, r);
      const float d = s[yy * w + xx];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float P = d * r[c];
        gx[c] += kSX[i][j] * P;
        gy[c] += kSY[i][j] * P;
      }
    }
  }
}

__device__ __forceinline__ void cross3(const float a[3], const float b[3], float c[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

__global__ __launch_bounds__(kT) void sr_normals_kernel(NormParams p) {
  const int hw = p.h * p.w;
  const int pix = blockIdx.x * kT + threadIdx.x;
  if (pix >= hw) return;
  const int b = blockIdx.y;
  const int y = pix / p.w, x = pix - y * p.w;
  float gx[3], gy[3], c[3];
  point_grads(p.s + (int64_t)b * hw, p.invK + b * 16, y, x, p.h, p.w, gx, gy);
  cross3(gx, gy, c);
  const float nrm = sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  const float den = clamp_min_nan(nrm, kNormEps);
  float* o = p.normals + (int64_t)b * 3 * hw + pix;
#pragma unroll
  for (int k = 0; k < 3; ++k) o[(int64_t)k * hw] = c[k] / den;
}

// adjoint 1: d normals -> d c -> (d gx, d gy) per pixel
__global__ __launch_bounds__(kT) void sr_normals_bwd_grads_kernel(NormParams p) {
  const int hw = p.h * p.w;
  const int pix = blockIdx.x * kT + threadIdx.x;
  if (pix >= hw) return;
  const int b = blockIdx.y;
  const int y = pix / p.w, x = pix - y * p.w;
  float gx[3], gy[3], c[3], g[3], dc[3], dgx[3], dgy[3];
  point_grads(p.s + (int64_t)b * hw, p.invK + b * 16, y, x, p.h, p.w, gx, gy);
  cross3(gx, gy, c);
  const float nrm = sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
  const float* gi = p.gn + (int64_t)b * 3 * hw + pix;
#pragma unroll
  for (int k = 0; k < 3; ++k) g[k] = gi[(int64_t)k * hw];
  if (nrm >= kNormEps) {
    // n = c / |c|: dc = (g - n (n . g)) / |c|
    const float n0 = c[0] / nrm, n1 = c[1] / nrm, n2 = c[2] / nrm;
    const float ng = n0 * g[0] + n1 * g[1] + n2 * g[2];
    dc[0] = (g[0] - n0 * ng) / nrm;
    dc[1] = (g[1] - n1 * ng) / nrm;
    dc[2] = (g[2] - n2 * ng) / nrm;
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) dc[k] = g[k] / kNormEps;
  }
  cross3(gy, dc, dgx);   // c = gx x gy: d gx = gy x dc, d gy = dc x gx
  cross3(dc, gx, dgy);
  float* o = p.dG + (int64_t)b * 6 * hw + pix;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    o[(int64_t)k * hw] = dgx[k];
    o[(int64_t)(3 + k) * hw] = dgy[k];
  }
}

// adjoint 2: gather the Sobel adjoint (replicate borders) into d points, then d blurred depth = d points . ray
__global__ __launch_bounds__(kT) void sr_normals_bwd_points_kernel(NormParams p) {
  const int hw = p.h * p.w;
  const int pix = blockIdx.x * kT + threadIdx.x;
  if (pix >= hw) return;
  const int b = blockIdx.y;
  const int y = pix / p.w, x = pix - y * p.w;
  const float* dG = p.dG + (int64_t)b * 6 * hw;
  float acc[3] = {0.0f, 0.0f, 0.0f};
  for (int py = max(y - 1, 0); py <= min(y + 1, p.h - 1); ++py) {
    for (int px = max(x - 1, 0); px <= min(x + 1, p.w - 1); ++px) {
      const int pp = py * p.w + px;
      float dgx[3], dgy[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        dgx[k] = dG[(int64_t)k * hw + pp];
        dgy[k] = dG[(int64_t)(3 + k) * hw + pp];
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        if (clampi(py + i - 1, 0, p.h - 1) != y) continue;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          if (clampi(px + j - 1, 0, p.w - 1) != x) continue;
#pragma unroll
          for (int k = 0; k < 3; ++k) acc[k] += kSX[i][j] * dgx[k] + kSY[i][j] * dgy[k];
        }
      }
    }
  }
  float r[3];
  ray(p.invK + b * 16, x, y, r);
  p.ds[(int64_t)b * hw + pix] = acc[0] * r[0] + acc[1] * r[1] + acc[2] * r[2];
}

// adjoint 3: the blur's adjoint (reflect padding), per axis the sum of the taps that land on this pixel
__global__ __launch_bounds__(kT) void sr_normals_bwd_blur_kernel(NormParams p) {
  const int hw = p.h * p.w;
  const int pix = blockIdx.x * kT + threadIdx.x;
  if (pix >= hw) return;
  const int b = blockIdx.y;
  const int y = pix / p.w, x = pix - y * p.w;
  float ay[5], ax[5];
#pragma unroll
  for (int d = 0; d < 5; ++d) {
    const int qy = y + d - 2, qx = x + d - 2;
    float sy = 0.0f, sx = 0.0f;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      if (qy >= 0 && qy < p.h && reflecti(qy + t - 2, p.h) == y) sy += p.g[t];
      if (qx >= 0 && qx < p.w && reflecti(qx + t - 2, p.w) == x) sx += p.g[t];
    }
    ay[d] = sy;
    ax[d] = sx;
  }
  const float* ds = p.ds + (int64_t)b * hw;
  float acc = 0.0f;
#pragma unroll
  for (int dy = 0; dy < 5; ++dy) {
    const int qy = y + dy - 2;
    if (qy < 0 || qy >= p.h) continue;
#pragma unroll
    for (int dx = 0; dx < 5; ++dx) {
      const int qx = x + dx - 2;
      if (qx < 0 || qx >= p.w) continue;
      acc += (ay[dy] * ax[dx]) * ds[qy * p.w + qx];
    }
  }
  p.gdepth[(int64_t)b * hw + pix] = acc;
}

void gauss5(float g[5]) {
  double e[5], s = 0.0;
  for (int t = 0; t < 5; ++t) s += (e[t] = exp(-(double)((t - 2) * (t - 2)) / 8.0));
  for (int t = 0; t < 5; ++t) g[t] = (float)(e[t] / s);
}

bool maps_ok(int B, int h, int w) {
  return B >= 1 && h >= 3 && w >= 3 && B <= 65535 && (int64_t)h * w <= INT32_MAX / 8;
}

// ---------------------------------------------------------------------------------------- normals loss --------------
__global__ __launch_bounds__(kT) void sr_normals_loss_kernel(const float* __restrict__ ng, const float* __restrict__ np,
                                                             int hw, float* __restrict__ partials) {
  const int pix = blockIdx.x * kT + threadIdx.x;
  const int b = blockIdx.y;
  float v[kNormalsFields] = {0.0f, 0.0f};
  if (pix < hw) {
    const int64_t o = (int64_t)b * 3 * hw + pix;
    const float g0 = ng[o], g1 = ng[o + hw], g2 = ng[o + 2 * (int64_t)hw];
    const float p0 = np[o], p1 = np[o + hw], p2 = np[o + 2 * (int64_t)hw];
    const bool m = __builtin_isfinite(g0) & __builtin_isfinite(g1) & __builtin_isfinite(g2) &
                   __builtin_isfinite(p0) & __builtin_isfinite(p1) & __builtin_isfinite(p2);
    if (m) {
      v[0] = 0.5f * (1.0f - (p0 * g0 + p1 * g1 + p2 * g2));
      v[1] = 1.0f;
    }
  }
  store_partials<kNormalsFields>(v, partials, (int64_t)b * gridDim.x + blockIdx.x);
}

__global__ __launch_bounds__(kT) void sr_normals_loss_bwd_kernel(const float* __restrict__ gout,
                                                                 const float* __restrict__ stats,
                                                                 const float* __restrict__ ng,
                                                                 const float* __restrict__ np, int hw,
                                                                 float* __restrict__ gp) {
  const int pix = blockIdx.x * kT + threadIdx.x;
  if (pix >= hw) return;
  const int64_t o = (int64_t)blockIdx.y * 3 * hw + pix;
  const float cnt = stats[1];
  const float s = cnt > 0.0f ? gout[0] / cnt : 0.0f;
  float g[3], q[3];
  bool m = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    g[k] = ng[o + k * (int64_t)hw];
    q[k] = np[o + k * (int64_t)hw];
    m = m & __builtin_isfinite(g[k]) & __builtin_isfinite(q[k]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) gp[o + k * (int64_t)hw] = m ? -0.5f * s * g[k] : 0.0f;
}

// ------------------------------------------------------------------------------------------- grad loss --------------
struct Pyr {
  int h[4], w[4];
  int64_t off[4];   // offsets of levels 1..3 in the level buffers (entry 0 unused)
};

Pyr pyramid(int h, int w) {
  Pyr P;
  P.h[0] = h;
  P.w[0] = w;
  P.off[0] = 0;
  int64_t o = 0;
  for (int l = 1; l < 4; ++l) {
    P.h[l] = (P.h[l - 1] + 1) / 2;
    P.w[l] = (P.w[l - 1] + 1) / 2;
    P.off[l] = o;
    o += (int64_t)P.h[l] * P.w[l];
  }
  P.off[0] = o;   // per-image floats of levels 1..3
  return P;
}

struct GradParams {
  const float* gt[4];
  const float* pred[4];
  float* dl[4];      // adjoints of levels 0..3 (0: the output gradient)
  int h[4], w[4];
  int64_t bstride[4];   // per-image stride of each level's buffer
  const float* gout;
  const float* stats;
  float* partials;
};

// level l+1 of gt (z = 0) and pred (z = 1) from level l: zero padding 1, stride 2
__global__ __launch_bounds__(kT) void sr_blurpool_kernel(GradParams p, int l) {
  const int ho = p.h[l + 1], wo = p.w[l + 1], hi = p.h[l], wi = p.w[l];
  const int pix = blockIdx.x * kT + threadIdx.x;
  if (pix >= ho * wo) return;
  const int b = blockIdx.y;
  const float* in = (blockIdx.z == 0 ? p.gt[l] : p.pred[l]) + (int64_t)b * p.bstride[l];
  float* out = const_cast<float*>(blockIdx.z == 0 ? p.gt[l + 1] : p.pred[l + 1]) + (int64_t)b * p.bstride[l + 1];
  const int y = pix / wo, x = pix - y * wo;
  float acc = 0.0f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int yy = 2 * y + i - 1;
    if (yy < 0 || yy >= hi) continue;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int xx = 2 * x + j - 1;
      if (xx < 0 || xx >= wi) continue;
      acc += (kBP[i] * kBP[j] / 16.0f) * in[yy * wi + xx];
    }
  }
  out[pix] = acc;
}

__device__ __forceinline__ void sobel_at(const float* __restrict__ m, int y, int x, int h, int w, float& gx, float& gy) {
  gx = gy = 0.0f;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const int yy = clampi(y + i - 1, 0, h - 1);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float v = m[yy * w + clampi(x + j - 1, 0, w - 1)];
      gx += kSX[i][j] * v;
      gy += kSY[i][j] * v;
    }
  }
}

// masked |grad pred - grad gt| of every level: z = level, partial fields (sum, count) of that level, zeros elsewhere
__global__ __launch_bounds__(kT) void sr_grad_loss_kernel(GradParams p) {
  const int l = blockIdx.z, h = p.h[l], w = p.w[l];
  const int pix = blockIdx.x * kT + threadIdx.x;
  const int b = blockIdx.y;
  float v[kGradFields];
#pragma unroll
  for (int f = 0; f < kGradFields; ++f) v[f] = 0.0f;
  if (pix < h * w) {
    const int y = pix / w, x = pix - y * w;
    float gxg, gyg, gxp, gyp;
    sobel_at(p.gt[l] + (int64_t)b * p.bstride[l], y, x, h, w, gxg, gyg);
    sobel_at(p.pred[l] + (int64_t)b * p.bstride[l], y, x, h, w, gxp, gyp);
    float s = 0.0f, c = 0.0f;
    if (__builtin_isfinite(gxg)) { s += __builtin_fabsf(gxp - gxg); c += 1.0f; }
    if (__builtin_isfinite(gyg)) { s += __builtin_fabsf(gyp - gyg); c += 1.0f; }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (k == l) { v[2 * k] = s; v[2 * k + 1] = c; }
  }
  store_partials<kGradFields>(v, p.partials, ((int64_t)l * gridDim.y + b) * gridDim.x + blockIdx.x);
}

// adjoint of level l: its own masked-L1 Sobel term plus the blur-pool adjoint of level l+1's adjoint
__global__ __launch_bounds__(kT) void sr_grad_loss_bwd_kernel(GradParams p, int l) {
  const int h = p.h[l], w = p.w[l];
  const int pix = blockIdx.x * kT + threadIdx.x;
  if (pix >= h * w) return;
  const int b = blockIdx.y;
  const int y = pix / w, x = pix - y * w;
  const float* G = p.gt[l] + (int64_t)b * p.bstride[l];
  const float* Q = p.pred[l] + (int64_t)b * p.bstride[l];
  const float cnt = p.stats[1 + l];
  const float sc = cnt > 0.0f ? p.gout[0] / cnt : 0.0f;
  float acc = 0.0f;
  for (int py = max(y - 1, 0); py <= min(y + 1, h - 1); ++py) {
    for (int px = max(x - 1, 0); px <= min(x + 1, w - 1); ++px) {
      float gxg, gyg, gxp, gyp;
      sobel_at(G, py, px, h, w, gxg, gyg);
      sobel_at(Q, py, px, h, w, gxp, gyp);
      const float sx = __builtin_isfinite(gxg) ? sgnf(gxp - gxg) : 0.0f;
      const float sy = __builtin_isfinite(gyg) ? sgnf(gyp - gyg) : 0.0f;
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        if (clampi(py + i - 1, 0, h - 1) != y) continue;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          if (clampi(px + j - 1, 0, w - 1) != x) continue;
          acc += kSX[i][j] * sx + kSY[i][j] * sy;
        }
      }
    }
  }
  acc *= sc;
  if (l < 3) {
    const int hn = p.h[l + 1], wn = p.w[l + 1];
    const float* dn = p.dl[l + 1] + (int64_t)b * p.bstride[l + 1];
    float up = 0.0f;
    // level l+1 pixel j reads level l pixels 2j-1 .. 2j+1
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const int t = y + 1 - i;
      if (t < 0 || (t & 1) || (t >> 1) >= hn) continue;
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int u = x + 1 - j;
        if (u < 0 || (u & 1) || (u >> 1) >= wn) continue;
        up += (kBP[i] * kBP[j] / 16.0f) * dn[(t >> 1) * wn + (u >> 1)];
      }
    }
    acc += up;
  }
  p.dl[l][(int64_t)b * p.bstride[l] + pix] = acc;
}

size_t grad_partials_floats(int B, int h, int w) { return (size_t)4 * B * blocks_for((int64_t)h * w) * kGradFields; }

// ------------------------------------------------------------------------------------------- multi-view -------------
struct MVParams {
  const float* pred;     // [B,h,w]
  const float* gt;       // [B,h,w]
  const float* src;      // [B,K,h,w]
  const float* invK;     // [B,4,4]
  const float* srcK;     // [B,K,4,4]
  const float* wTc;      // [B,4,4]
  const float* cTw;      // [B,K,4,4]
  const float* gout;
  const float* stats;
  float* partials;
  uint8_t* valid;        // optional [B,K,h,w]
  float* sampled;        // optional [B,K,h,w]
  float* gpred;          // [B,h,w]
  int K, h, w;
  float eps;
};

struct MVPix {
  float zq, zp, s, dzdd;
  bool valid;
};

// (u, v) -> world point of depth d: T_wc (d * invK[:3,:3] (u + .5, v + .5, 1), 1)
__device__ __forceinline__ void mv_world(const float* __restrict__ iK, const float* __restrict__ T, float d, int x, int y,
                                         float wp[4], float rw[4]) {
  float r[3];
  ray(iK, x, y, r);
  const float c0 = d * r[0], c1 = d * r[1], c2 = d * r[2];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    wp[i] = T[i * 4 + 0] * c0 + T[i * 4 + 1] * c1 + T[i * 4 + 2] * c2 + T[i * 4 + 3];
    rw[i] = T[i * 4 + 0] * r[0] + T[i * 4 + 1] * r[1] + T[i * 4 + 2] * r[2];   // d world / d d
  }
}

__device__ __forceinline__ MVPix mv_pixel(const MVParams& p, int b, int k, int x, int y, const float wg[4],
                                          const float wq[4], const float rq[4]) {
  const float* Kk = p.srcK + ((int64_t)b * p.K + k) * 16;
  const float* Tk = p.cTw + ((int64_t)b * p.K + k) * 16;
  float P[3][4];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
      P[i][j] = Kk[i * 4 + 0] * Tk[0 * 4 + j] + Kk[i * 4 + 1] * Tk[1 * 4 + j] + Kk[i * 4 + 2] * Tk[2 * 4 + j] +
                Kk[i * 4 + 3] * Tk[3 * 4 + j];
  float q[3], qp = 0.0f, dz = 0.0f;
#pragma unroll
  for (int i = 0; i < 3; ++i) q[i] = P[i][0] * wg[0] + P[i][1] * wg[1] + P[i][2] * wg[2] + P[i][3] * wg[3];
  qp = P[2][0] * wq[0] + P[2][1] * wq[1] + P[2][2] * wq[2] + P[2][3] * wq[3];
  dz = P[2][0] * rq[0] + P[2][1] * rq[1] + P[2][2] * rq[2] + P[2][3] * rq[3];
  MVPix r;
  r.zq = q[2] + p.eps;
  r.zp = qp + p.eps;
  r.dzdd = dz;
  const float sc = __builtin_fabsf(q[2]) > p.eps ? 1.0f / r.zq : 1.0f;
  const float px = q[0] * sc, py = q[1] * sc;
  // grid_sample(nearest, align_corners=False, zeros): normalise to [-1, 1] and back, then round half to even
  const float fw = (float)p.w, fh = (float)p.h;
  const float gx = 2.0f * (px / fw) - 1.0f, gy = 2.0f * (py / fh) - 1.0f;
  const float ix = __builtin_rintf(((gx + 1.0f) * fw - 1.0f) / 2.0f);
  const float iy = __builtin_rintf(((gy + 1.0f) * fh - 1.0f) / 2.0f);
  float s = 0.0f;
  if (ix >= 0.0f && ix <= fw - 1.0f && iy >= 0.0f && iy <= fh - 1.0f)
    s = p.src[((int64_t)b * p.K + k) * p.h * p.w + (int)iy * p.w + (int)ix];
  r.s = s;
  r.valid = (r.zq < 1.05f * s) & (r.zq > 0.0f) & (s > 0.0f);
  return r;
}

__global__ __launch_bounds__(kT) void sr_mv_loss_kernel(MVParams p) {
  const int hw = p.h * p.w;
  const int pix = blockIdx.x * kT + threadIdx.x;
  const int b = blockIdx.y;
  float v[kMVFields];
#pragma unroll
  for (int f = 0; f < kMVFields; ++f) v[f] = 0.0f;
  if (pix < hw) {
    const int y = pix / p.w, x = pix - y * p.w;
    float wg[4], wq[4], rg[4], rq[4];
    mv_world(p.invK + b * 16, p.wTc + b * 16, p.gt[(int64_t)b * hw + pix], x, y, wg, rg);
    mv_world(p.invK + b * 16, p.wTc + b * 16, p.pred[(int64_t)b * hw + pix], x, y, wq, rq);
#pragma unroll
    for (int k = 0; k < SR_LOSS_MAX_SOURCES; ++k) {
      if (k >= p.K) break;
      const MVPix r = mv_pixel(p, b, k, x, y, wg, wq, rq);
      const int64_t o = ((int64_t)b * p.K + k) * hw + pix;
      if (p.valid) p.valid[o] = r.valid ? 1 : 0;
      if (p.sampled) p.sampled[o] = r.s;
      const float e = __builtin_fabsf(logf(r.s) - logf(r.zp));
      if (r.valid && !__builtin_isnan(e)) {
        v[2 * k] = e;
        v[2 * k + 1] = 1.0f;
      }
    }
  }
  // the pairs of sources k >= K stay zero and are not read by the finalize
  store_partials<kMVFields>(v, p.partials, (int64_t)b * gridDim.x + blockIdx.x);
}

__global__ __launch_bounds__(kT) void sr_mv_loss_bwd_kernel(MVParams p) {
  const int hw = p.h * p.w;
  const int pix = blockIdx.x * kT + threadIdx.x;
  if (pix >= hw) return;
  const int b = blockIdx.y;
  const int y = pix / p.w, x = pix - y * p.w;
  float wg[4], wq[4], rg[4], rq[4];
  mv_world(p.invK + b * 16, p.wTc + b * 16, p.gt[(int64_t)b * hw + pix], x, y, wg, rg);
  mv_world(p.invK + b * 16, p.wTc + b * 16, p.pred[(int64_t)b * hw + pix], x, y, wq, rq);
  const float g = p.gout[0] / (float)p.K;
  float acc = 0.0f;
  for (int k = 0; k < p.K; ++k) {
    const MVPix r = mv_pixel(p, b, k, x, y, wg, wq, rq);
    const float lz = logf(r.zp);
    const float e = __builtin_fabsf(logf(r.s) - lz);
    const float cnt = p.stats[1 + k];
    if (r.valid && !__builtin_isnan(e) && cnt > 0.0f) acc += (g / cnt) * sgnf(lz - logf(r.s)) / r.zp * r.dzdd;
  }
  p.gpred[(int64_t)b * hw + pix] = acc;
}

// ------------------------------------------------------------------------------------------ depth terms -------------
struct DepthParams {
  const float* gt;      // [B,h,w]
  const uint8_t* mask;  // [B,h,w]
  const float* pred;    // [B,h,w] depth
  const float* lg[4];   // log depth scales (NULL: absent); lg[0] is [B,h,w]
  int hs[4], ws[4];
  int h, w, present, gt_is_log;
  float lambda;
  const float* gouts;   // [5]: ms, abs, inv_abs, log_l1, si
  const float* stats;
  float* partials;
  float* gpred;
  float* glg[4];
};

__global__ __launch_bounds__(kT) void sr_depth_terms_kernel(DepthParams p) {
  const int hw = p.h * p.w;
  const int pix = blockIdx.x * kT + threadIdx.x;
  const int b = blockIdx.y;
  float v[kDepthFields];
#pragma unroll
  for (int f = 0; f < kDepthFields; ++f) v[f] = 0.0f;
  if (pix < hw && p.mask[(int64_t)b * hw + pix]) {
    const int y = pix / p.w, x = pix - y * p.w;
    const float gt = p.gt[(int64_t)b * hw + pix];
    const float lgt = p.gt_is_log ? gt : logf(gt);
    const float pr = p.pred[(int64_t)b * hw + pix];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (!(p.present >> i & 1)) continue;
      const int sy = sr_nearest_src(y, p.hs[i], p.h), sx = sr_nearest_src(x, p.ws[i], p.w);
      v[i] = __builtin_fabsf(lgt - p.lg[i][((int64_t)b * p.hs[i] + sy) * p.ws[i] + sx]);
    }
    v[4] = 1.0f;
    v[5] = __builtin_fabsf(gt - pr);
    if (pr > 0.1f) {
      v[6] = __builtin_fabsf(1.0f / gt - 1.0f / pr);
      v[7] = 1.0f;
    }
    const float l0 = p.lg[0][(int64_t)b * hw + pix];
    v[8] = __builtin_fabsf(lgt - l0);
    const float d = lgt - l0;
    v[9] = d;
    v[10] = d * d;
  }
  store_partials<kDepthFields>(v, p.partials, (int64_t)b * gridDim.x + blockIdx.x);
}

// z = 0: d depth_pred (abs, inv_abs); z = 1 + i: d log scale i (ms term; scale 0 also si and log l1)
__global__ __launch_bounds__(kT) void sr_depth_terms_bwd_kernel(DepthParams p) {
  const int t = blockIdx.z;
  const int b = blockIdx.y;
  const int pix = blockIdx.x * kT + threadIdx.x;
  const int hw = p.h * p.w;
  const float n = p.stats[5], ni = p.stats[6];
  if (t == 0) {
    if (pix >= hw) return;
    const int64_t o = (int64_t)b * hw + pix;
    float g = 0.0f;
    if (p.mask[o]) {
      const float gt = p.gt[o], pr = p.pred[o];
      g = p.gouts[1] / n * sgnf(pr - gt);
      if (pr > 0.1f) {
        const float rp = 1.0f / pr;
        g += p.gouts[2] / ni * (sgnf(rp - 1.0f / gt) * -(rp * rp));
      }
    }
    p.gpred[o] = g;
    return;
  }
  const int i = t - 1;
  if (!(p.present >> i & 1)) return;
  const int hi = p.hs[i], wi = p.ws[i];
  if (pix >= hi * wi) return;
  const int cy = pix / wi, cx = pix - cy * wi;
  const float* L = p.lg[i];
  const int64_t co = (int64_t)b * hi * wi + pix;
  const float lv = L[co];
  // the fine rows / columns whose nearest source is (cy, cx): a contiguous range, the mapping being monotone
  int y0 = (int)((int64_t)cy * p.h / hi);
  while (y0 > 0 && sr_nearest_src(y0 - 1, hi, p.h) >= cy) --y0;
  while (y0 < p.h && sr_nearest_src(y0, hi, p.h) < cy) ++y0;
  int x0 = (int)((int64_t)cx * p.w / wi);
  while (x0 > 0 && sr_nearest_src(x0 - 1, wi, p.w) >= cx) --x0;
  while (x0 < p.w && sr_nearest_src(x0, wi, p.w) < cx) ++x0;
  float ms = 0.0f, si = 0.0f, l1 = 0.0f;
  const float md = p.stats[7], siv = p.stats[4];
  for (int y = y0; y < p.h && sr_nearest_src(y, hi, p.h) == cy; ++y) {
    for (int x = x0; x < p.w && sr_nearest_src(x, wi, p.w) == cx; ++x) {
      const int64_t o = (int64_t)b * hw + y * p.w + x;
      if (!p.mask[o]) continue;
      const float lgt = p.gt_is_log ? p.gt[o] : logf(p.gt[o]);
      ms += sgnf(lv - lgt);
      if (i == 0) {
        // s0 is at gt size: (y, x) is this pixel
        const float d = lgt - lv;
        si += -(d - p.lambda * md);
        l1 += sgnf(lv - lgt);
      }
    }
  }
  float g = p.gouts[0] / (float)(1 << i) / n * ms;
  if (i == 0) g += p.gouts[4] * si / (n * siv) + p.gouts[3] / n * l1;
  p.glg[i][co] = g;
}

}  // namespace

// ====================================================================================================================
extern "C" size_t sr_normals_workspace_bytes(int B, int h, int w) {
  if (!maps_ok(B, h, w)) return 0;
  return (size_t)8 * B * h * w * sizeof(float);
}

extern "C" int sr_normals_fwd(const float* depth, const float* invK, int B, int h, int w, float* normals, void* scratch,
                              size_t scratch_bytes, void* stream) {
  if (!depth || !invK || !normals || !scratch || !maps_ok(B, h, w)) return SR_ERR_INVALID_ARGUMENT;
  if (scratch_bytes < sr_normals_workspace_bytes(B, h, w)) return SR_ERR_WORKSPACE_TOO_SMALL;
  NormParams P{};
  P.depth = depth; P.invK = invK; P.s = (float*)scratch; P.normals = normals;
  P.h = h; P.w = w;
  gauss5(P.g);
  const dim3 grid(blocks_for((int64_t)h * w), B);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sr_normals_blur_kernel, grid, dim3(kT), 0, st, P);
  hipLaunchKernelGGL(sr_normals_kernel, grid, dim3(kT), 0, st, P);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_normals_bwd(const float* grad_normals, const float* depth, const float* invK, int B, int h, int w,
                              float* grad_depth, void* scratch, size_t scratch_bytes, void* stream) {
  if (!grad_normals || !depth || !invK || !grad_depth || !scratch || !maps_ok(B, h, w)) return SR_ERR_INVALID_ARGUMENT;
  if (scratch_bytes < sr_normals_workspace_bytes(B, h, w)) return SR_ERR_WORKSPACE_TOO_SMALL;
  const int64_t n = (int64_t)B * h * w;
  NormParams P{};
  P.depth = depth; P.invK = invK; P.gn = grad_normals; P.gdepth = grad_depth;
  P.s = (float*)scratch; P.dG = P.s + n; P.ds = P.dG + 6 * n;
  P.h = h; P.w = w;
  gauss5(P.g);
  const dim3 grid(blocks_for((int64_t)h * w), B);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sr_normals_blur_kernel, grid, dim3(kT), 0, st, P);
  hipLaunchKernelGGL(sr_normals_bwd_grads_kernel, grid, dim3(kT), 0, st, P);
  hipLaunchKernelGGL(sr_normals_bwd_points_kernel, grid, dim3(kT), 0, st, P);
  hipLaunchKernelGGL(sr_normals_bwd_blur_kernel, grid, dim3(kT), 0, st, P);
  return sr_hip_rc(hipGetLastError());
}

extern "C" size_t sr_normals_loss_workspace_bytes(int B, int h, int w) {
  if (!maps_ok(B, h, w)) return 0;
  return (size_t)B * blocks_for((int64_t)h * w) * kNormalsFields * sizeof(float);
}

extern "C" int sr_normals_loss_fwd(const float* normals_gt, const float* normals_pred, int B, int h, int w, float* out,
                                   void* scratch, size_t scratch_bytes, void* stream) {
  if (!normals_gt || !normals_pred || !out || !scratch || !maps_ok(B, h, w)) return SR_ERR_INVALID_ARGUMENT;
  if (scratch_bytes < sr_normals_loss_workspace_bytes(B, h, w)) return SR_ERR_WORKSPACE_TOO_SMALL;
  const dim3 grid(blocks_for((int64_t)h * w), B);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sr_normals_loss_kernel, grid, dim3(kT), 0, st, normals_gt, normals_pred, h * w, (float*)scratch);
  int rc = sr_hip_rc(hipGetLastError());
  if (rc) return rc;
  return finalize((const float*)scratch, (int64_t)grid.x * B, kNormalsFields, kNormalsFields, kFinNormals, 0, 0, 0.0f, out, st);
}

extern "C" int sr_normals_loss_bwd(const float* grad_out, const float* stats, const float* normals_gt,
                                   const float* normals_pred, int B, int h, int w, float* grad_pred, void* stream) {
  if (!grad_out || !stats || !normals_gt || !normals_pred || !grad_pred || !maps_ok(B, h, w))
    return SR_ERR_INVALID_ARGUMENT;
  const dim3 grid(blocks_for((int64_t)h * w), B);
  hipLaunchKernelGGL(sr_normals_loss_bwd_kernel, grid, dim3(kT), 0, (hipStream_t)stream, grad_out, stats, normals_gt,
                     normals_pred, h * w, grad_pred);
  return sr_hip_rc(hipGetLastError());
}

extern "C" size_t sr_grad_loss_workspace_bytes(int B, int h, int w) {
  if (!maps_ok(B, h, w)) return 0;
  const Pyr P = pyramid(h, w);
  // levels 1..3 of gt, pred and of the adjoint, then the partials
  return ((size_t)3 * B * P.off[0] + grad_partials_floats(B, h, w)) * sizeof(float);
}

static GradParams grad_params(const float* gt, const float* pred, int B, int h, int w, void* scratch) {
  const Pyr Y = pyramid(h, w);
  const int64_t lvl = (int64_t)B * Y.off[0];
  float* base = (float*)scratch;
  GradParams p{};
  for (int l = 0; l < 4; ++l) {
    p.h[l] = Y.h[l];
    p.w[l] = Y.w[l];
    if (l == 0) {
      p.gt[0] = gt;
      p.pred[0] = pred;
      p.bstride[0] = (int64_t)h * w;
    } else {
      p.gt[l] = base + (int64_t)B * Y.off[l];
      p.pred[l] = base + lvl + (int64_t)B * Y.off[l];
      p.dl[l] = base + 2 * lvl + (int64_t)B * Y.off[l];
      p.bstride[l] = (int64_t)Y.h[l] * Y.w[l];
    }
  }
  p.partials = base + 3 * lvl;
  return p;
}

extern "C" int sr_grad_loss_fwd(const float* depth_gt, const float* depth_pred, int B, int h, int w, float* out,
                                void* scratch, size_t scratch_bytes, void* stream) {
  if (!depth_gt || !depth_pred || !out || !scratch || !maps_ok(B, h, w)) return SR_ERR_INVALID_ARGUMENT;
  if (scratch_bytes < sr_grad_loss_workspace_bytes(B, h, w)) return SR_ERR_WORKSPACE_TOO_SMALL;
  GradParams p = grad_params(depth_gt, depth_pred, B, h, w, scratch);
  hipStream_t st = (hipStream_t)stream;
  for (int l = 0; l < 3; ++l)
    hipLaunchKernelGGL(sr_blurpool_kernel, dim3(blocks_for((int64_t)p.h[l + 1] * p.w[l + 1]), B, 2), dim3(kT), 0, st,
                       p, l);
  const dim3 grid(blocks_for((int64_t)h * w), B, 4);
  hipLaunchKernelGGL(sr_grad_loss_kernel, grid, dim3(kT), 0, st, p);
  int rc = sr_hip_rc(hipGetLastError());
  if (rc) return rc;
  return finalize(p.partials, (int64_t)grid.x * B * 4, kGradFields, kGradFields, kFinGrad, 0, 0, 0.0f, out, st);
}

extern "C" int sr_grad_loss_bwd(const float* grad_out, const float* stats, const float* depth_gt,
                                const float* depth_pred, int B, int h, int w, float* grad_pred, void* scratch,
                                size_t scratch_bytes, void* stream) {
  if (!grad_out || !stats || !depth_gt || !depth_pred || !grad_pred || !scratch || !maps_ok(B, h, w))
    return SR_ERR_INVALID_ARGUMENT;
  if (scratch_bytes < sr_grad_loss_workspace_bytes(B, h, w)) return SR_ERR_WORKSPACE_TOO_SMALL;
  GradParams p = grad_params(depth_gt, depth_pred, B, h, w, scratch);
  p.dl[0] = grad_pred;
  p.gout = grad_out;
  p.stats = stats;
  hipStream_t st = (hipStream_t)stream;
  for (int l = 3; l >= 0; --l)
    hipLaunchKernelGGL(sr_grad_loss_bwd_kernel, dim3(blocks_for((int64_t)p.h[l] * p.w[l]), B), dim3(kT), 0, st, p, l);
  return sr_hip_rc(hipGetLastError());
}

extern "C" size_t sr_mv_loss_workspace_bytes(int B, int K, int h, int w) {
  if (!maps_ok(B, h, w) || K < 1 || K > SR_LOSS_MAX_SOURCES) return 0;
  return (size_t)B * blocks_for((int64_t)h * w) * kMVFields * sizeof(float);
}

static bool mv_args_ok(const float* pred, const float* gt, const float* src, const float* invK, const float* srcK,
                       const float* wTc, const float* cTw, int B, int K, int h, int w) {
  return pred && gt && src && invK && srcK && wTc && cTw && maps_ok(B, h, w) && K >= 1 && K <= SR_LOSS_MAX_SOURCES &&
         (int64_t)K * h * w <= INT32_MAX;
}

extern "C" int sr_mv_loss_fwd(const float* depth_pred, const float* depth_gt, const float* src_depth,
                              const float* cur_invK, const float* src_K, const float* cur_world_T_cam,
                              const float* src_cam_T_world, int B, int K, int h, int w, float eps, float* out,
                              uint8_t* valid_mask, float* sampled, void* scratch, size_t scratch_bytes, void* stream) {
  if (!mv_args_ok(depth_pred, depth_gt, src_depth, cur_invK, src_K, cur_world_T_cam, src_cam_T_world, B, K, h, w) ||
      !out || !scratch)
    return SR_ERR_INVALID_ARGUMENT;
  if (scratch_bytes < sr_mv_loss_workspace_bytes(B, K, h, w)) return SR_ERR_WORKSPACE_TOO_SMALL;
  MVParams P{};
  P.pred = depth_pred; P.gt = depth_gt; P.src = src_depth; P.invK = cur_invK; P.srcK = src_K;
  P.wTc = cur_world_T_cam; P.cTw = src_cam_T_world; P.partials = (float*)scratch;
  P.valid = valid_mask; P.sampled = sampled;
  P.K = K; P.h = h; P.w = w; P.eps = eps;
  const dim3 grid(blocks_for((int64_t)h * w), B);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sr_mv_loss_kernel, grid, dim3(kT), 0, st, P);
  int rc = sr_hip_rc(hipGetLastError());
  if (rc) return rc;
  return finalize(P.partials, (int64_t)grid.x * B, 2 * K, kMVFields, kFinMV, K, 0, 0.0f, out, st);
}

extern "C" int sr_mv_loss_bwd(const float* grad_out, const float* stats, const float* depth_pred, const float* depth_gt,
                              const float* src_depth, const float* cur_invK, const float* src_K,
                              const float* cur_world_T_cam, const float* src_cam_T_world, int B, int K, int h, int w,
                              float eps, float* grad_pred, void* stream) {
  if (!mv_args_ok(depth_pred, depth_gt, src_depth, cur_invK, src_K, cur_world_T_cam, src_cam_T_world, B, K, h, w) ||
      !grad_out || !stats || !grad_pred)
    return SR_ERR_INVALID_ARGUMENT;
  MVParams P{};
  P.pred = depth_pred; P.gt = depth_gt; P.src = src_depth; P.invK = cur_invK; P.srcK = src_K;
  P.wTc = cur_world_T_cam; P.cTw = src_cam_T_world; P.gout = grad_out; P.stats = stats; P.gpred = grad_pred;
  P.K = K; P.h = h; P.w = w; P.eps = eps;
  hipLaunchKernelGGL(sr_mv_loss_bwd_kernel, dim3(blocks_for((int64_t)h * w), B), dim3(kT), 0, (hipStream_t)stream, P);
  return sr_hip_rc(hipGetLastError());
}

extern "C" size_t sr_depth_terms_workspace_bytes(int B, int h, int w) {
  if (B < 1 || B > 65535 || h < 1 || w < 1 || (int64_t)h * w > INT32_MAX / 8) return 0;
  return (size_t)B * blocks_for((int64_t)h * w) * kDepthFields * sizeof(float);
}

static int depth_params(DepthParams& P, const float* depth_gt, const uint8_t* mask_b, const float* depth_pred,
                        const float* log0, const float* log1, int h1, int w1, const float* log2, int h2, int w2,
                        const float* log3, int h3, int w3, int B, int h, int w, float si_lambda, int gt_is_log) {
  if (!depth_gt || !mask_b || !depth_pred || !log0) return SR_ERR_INVALID_ARGUMENT;
  if (B < 1 || B > 65535 || h < 1 || w < 1 || (int64_t)h * w > INT32_MAX / 8) return SR_ERR_INVALID_ARGUMENT;
  P = DepthParams{};
  P.gt = depth_gt; P.mask = mask_b; P.pred = depth_pred;
  const float* lg[4] = {log0, log1, log2, log3};
  const int hs[4] = {h, h1, h2, h3}, ws[4] = {w, w1, w2, w3};
  for (int i = 0; i < 4; ++i) {
    P.lg[i] = lg[i];
    P.hs[i] = hs[i];
    P.ws[i] = ws[i];
    if (lg[i]) {
      if (hs[i] < 1 || ws[i] < 1 || hs[i] > h || ws[i] > w) return SR_ERR_INVALID_ARGUMENT;
      P.present |= 1 << i;
    }
  }
  P.h = h; P.w = w; P.lambda = si_lambda; P.gt_is_log = gt_is_log ? 1 : 0;
  return SR_OK;
}

extern "C" int sr_depth_terms_fwd(const float* depth_gt, const uint8_t* mask_b, const float* depth_pred,
                                  const float* log0, const float* log1, int h1, int w1, const float* log2, int h2,
                                  int w2, const float* log3, int h3, int w3, int B, int h, int w, float si_lambda,
                                  int gt_is_log, float* out, void* scratch, size_t scratch_bytes, void* stream) {
  DepthParams P;
  int rc = depth_params(P, depth_gt, mask_b, depth_pred, log0, log1, h1, w1, log2, h2, w2, log3, h3, w3, B, h, w,
                        si_lambda, gt_is_log);
  if (rc) return rc;
  if (!out || !scratch) return SR_ERR_INVALID_ARGUMENT;
  if (scratch_bytes < sr_depth_terms_workspace_bytes(B, h, w)) return SR_ERR_WORKSPACE_TOO_SMALL;
  P.partials = (float*)scratch;
  const dim3 grid(blocks_for((int64_t)h * w), B);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sr_depth_terms_kernel, grid, dim3(kT), 0, st, P);
  rc = sr_hip_rc(hipGetLastError());
  if (rc) return rc;
  return finalize(P.partials, (int64_t)grid.x * B, kDepthFields, kDepthFields, kFinDepth, 0, P.present, si_lambda, out, st);
}

extern "C" int sr_depth_terms_bwd(const float* grad_outs, const float* stats, const float* depth_gt,
                                  const uint8_t* mask_b, const float* depth_pred, const float* log0, const float* log1,
                                  int h1, int w1, const float* log2, int h2, int w2, const float* log3, int h3, int w3,
                                  int B, int h, int w, float si_lambda, int gt_is_log, float* grad_depth_pred, float* grad_log0,
                                  float* grad_log1, float* grad_log2, float* grad_log3, void* stream) {
  DepthParams P;
  int rc = depth_params(P, depth_gt, mask_b, depth_pred, log0, log1, h1, w1, log2, h2, w2, log3, h3, w3, B, h, w,
                        si_lambda, gt_is_log);
  if (rc) return rc;
  float* g[4] = {grad_log0, grad_log1, grad_log2, grad_log3};
  if (!grad_outs || !stats || !grad_depth_pred) return SR_ERR_INVALID_ARGUMENT;
  for (int i = 0; i < 4; ++i) {
    if ((P.present >> i & 1) && !g[i]) return SR_ERR_INVALID_ARGUMENT;
    P.glg[i] = g[i];
  }
  P.gouts = grad_outs; P.stats = stats; P.gpred = grad_depth_pred;
  hipLaunchKernelGGL(sr_depth_terms_bwd_kernel, dim3(blocks_for((int64_t)h * w), B, 5), dim3(kT), 0,
                     (hipStream_t)stream, P);
  return sr_hip_rc(hipGetLastError());
}
