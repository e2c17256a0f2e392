// sr_optim.hip -- the optimiser step of the training path (gfx950): multi-tensor AdamW with decoupled weight decay, for
// every parameter tensor of a model in two launches.  Rules: include/simplerecon_hip.h, section "optimiser"; the host side
// (tables, state, version counters) is simplerecon_amd/optim.py.
//
// Prologue: one thread per tensor advances the tensor's step count and derives its two bias-correction scalars in
// double, as torch does in Python floats.  Streaming pass: one workgroup per SR_ADAMW_CHUNK consecutive elements of one
// tensor; the workgroup finds its tensor in the chunk prefix table (ten steps for 778 tensors).  A tensor whose four
// arrays are all 16-byte aligned moves 16 bytes per lane and access, the last n % 4 elements and every other tensor
// move single floats: the same arithmetic either way.  The pass reads p, g, m, v and writes p, m, v: 28 bytes per
// element and nothing else, so it runs at the speed of memory and the arithmetic (IEEE sqrt and two divides) is free.
//
// Every element value is the chain of fp32 operations of torch's CPU kernels (mul, lerp, mul + addcmul, sqrt, div, add,
// addcdiv) with their roundings: lerp and addcmul end in one fused multiply-add each, as ATen's vectorised kernels do,
// everything else is rounded separately, so contraction is off for the whole file and the two fused operations are
// written out.  Results are elementwise: the same bytes on every run.
#include "sr_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kT = 256;
constexpr int kChunk = SR_ADAMW_CHUNK;
constexpr int kVecIters = kChunk / (4 * kT);   // 16-byte accesses per lane and array
constexpr int kIters = kChunk / kT;            // single floats per lane and array
static_assert(kChunk % (4 * kT) == 0, "a chunk is a whole number of 16-byte accesses per lane");

struct Group {
  double lr, beta1, beta2;        // for the prologue's bias corrections
  float decay;                    // float(1 - lr * weight_decay)
  float w1, beta2f, w2, eps;      // float(1 - beta1), float(beta2), float(1 - beta2), float(eps)
};

struct Groups {
  Group g[SR_ADAMW_MAX_GROUPS];
};

struct Tables {
  const uint64_t* p;              // [T] addresses
  const uint64_t* g;              // [T] addresses, 0 = no gradient this step
  const uint64_t* m;
  const uint64_t* v;
  const int64_t* numel;           // [T]
  const int32_t* chunk_start;     // [T + 1] prefix sums of ceil(numel / kChunk)
  const int32_t* group;           // [T]
  float* steps;                   // [T]
  float* scalars;                 // [T][2] = lr / bias_correction1, sqrt(bias_correction2)
};

__device__ __forceinline__ bool skipped(const float* found_inf) { return found_inf != nullptr && *found_inf != 0.0f; }

__global__ __launch_bounds__(kT) void sr_adamw_prologue_kernel(Tables tb, Groups groups, int T, const float* found_inf) {
  const int t = blockIdx.x * kT + threadIdx.x;
  if (t >= T || skipped(found_inf) || tb.g[t] == 0) return;
  const float step = tb.steps[t] + 1.0f;
  tb.steps[t] = step;
  const Group& h = groups.g[tb.group[t]];
  const double bc1 = 1.0 - pow(h.beta1, (double)step);
  const double bc2 = 1.0 - pow(h.beta2, (double)step);
  tb.scalars[2 * t] = (float)(h.lr / bc1);
  tb.scalars[2 * t + 1] = (float)sqrt(bc2);
}

struct Hyper {
  float decay, w1, beta2, w2, eps, neg_step_size, bc2_sqrt, grad_scale;
  bool scaled;
};

__device__ __forceinline__ void update(float& p, float g, float& m, float& v, const Hyper& h) {
  if (h.scaled) g = g / h.grad_scale;
  p = p * h.decay;
  const float d = g - m;
  m = h.w1 < 0.5f ? fmaf(h.w1, d, m) : fmaf(h.w1 - 1.0f, d, g);   // lerp(m, g, 1 - beta1)
  v = v * h.beta2;
  v = fmaf(h.w2 * g, g, v);
  const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
  p = p + (h.neg_step_size * m) / denom;
}

__global__ __launch_bounds__(kT) void sr_adamw_kernel(Tables tb, Groups groups, int T, const float* grad_scale,
                                                      const float* found_inf) {
  if (skipped(found_inf)) return;
  const int c = blockIdx.x;
  int lo = 0, hi = T;   // the last tensor whose first chunk is at or in front of c (tensors without elements have none)
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (tb.chunk_start[mid] <= c) lo = mid;
    else hi = mid;
  }
  const int t = lo;
  const float* __restrict__ g = (const float*)tb.g[t];
  if (g == nullptr) return;
  const int64_t off = (int64_t)(c - tb.chunk_start[t]) * kChunk;
  const int64_t left = tb.numel[t] - off;
  if (left <= 0) return;
  const int cnt = left < kChunk ? (int)left : kChunk;
  float* __restrict__ p = (float*)tb.p[t];
  float* __restrict__ m = (float*)tb.m[t];
  float* __restrict__ v = (float*)tb.v[t];
  const Group& G = groups.g[tb.group[t]];
  Hyper h;
  h.decay = G.decay, h.w1 = G.w1, h.beta2 = G.beta2f, h.w2 = G.w2, h.eps = G.eps;
  h.neg_step_size = -tb.scalars[2 * t];
  h.bc2_sqrt = tb.scalars[2 * t + 1];
  h.scaled = grad_scale != nullptr;
  h.grad_scale = h.scaled ? *grad_scale : 1.0f;
  g += off, p += off, m += off, v += off;
  const bool wide = ((tb.p[t] | tb.g[t] | tb.m[t] | tb.v[t]) & 15) == 0;   // (off is a multiple of kChunk)
  if (wide) {
    const int nvec = cnt >> 2;
    float4 P[kVecIters], Gr[kVecIters], M[kVecIters], V[kVecIters];
#pragma unroll
    for (int k = 0; k < kVecIters; ++k) {
      const int i = threadIdx.x + k * kT;
      if (i < nvec) {
        P[k] = ((const float4*)p)[i];
        Gr[k] = ((const float4*)g)[i];
        M[k] = ((const float4*)m)[i];
        V[k] = ((const float4*)v)[i];
      }
    }
#pragma unroll
    for (int k = 0; k < kVecIters; ++k) {
      const int i = threadIdx.x + k * kT;
      if (i < nvec) {
        update(P[k].x, Gr[k].x, M[k].x, V[k].x, h);
        update(P[k].y, Gr[k].y, M[k].y, V[k].y, h);
        update(P[k].z, Gr[k].z, M[k].z, V[k].z, h);
        update(P[k].w, Gr[k].w, M[k].w, V[k].w, h);
        ((float4*)p)[i] = P[k];
        ((float4*)m)[i] = M[k];
        ((float4*)v)[i] = V[k];
      }
    }
    const int i = (nvec << 2) + threadIdx.x;   // the tail of the tensor's last chunk: up to three floats
    if (threadIdx.x < 3 && i < cnt) {
      float pp = p[i], mm = m[i], vv = v[i];
      update(pp, g[i], mm, vv, h);
      p[i] = pp, m[i] = mm, v[i] = vv;
    }
  } else {
#pragma unroll 4
    for (int k = 0; k < kIters; ++k) {
      const int i = threadIdx.x + k * kT;
      if (i < cnt) {
        float pp = p[i], mm = m[i], vv = v[i];
        update(pp, g[i], mm, vv, h);
        p[i] = pp, m[i] = mm, v[i] = vv;
      }
    }
  }
}

}  // namespace

extern "C" int sr_adamw_step(const void* p_ptrs, const void* g_ptrs, const void* m_ptrs, const void* v_ptrs,
                             const int64_t* numel, const int32_t* chunk_start, const int32_t* group, float* steps,
                             float* scalars, int num_tensors, int num_chunks, const double* groups_host, int num_groups,
                             const float* grad_scale, const float* found_inf, void* stream) {
  if (!p_ptrs || !g_ptrs || !m_ptrs || !v_ptrs || !numel || !chunk_start || !group || !steps || !scalars || !groups_host)
    return SR_ERR_INVALID_ARGUMENT;
  if (num_tensors < 1 || num_chunks < 0 || num_groups < 1) return SR_ERR_INVALID_ARGUMENT;
  if (num_tensors > SR_ADAMW_MAX_TENSORS || num_groups > SR_ADAMW_MAX_GROUPS) return SR_ERR_UNSUPPORTED;
  if ((((uintptr_t)p_ptrs | (uintptr_t)g_ptrs | (uintptr_t)m_ptrs | (uintptr_t)v_ptrs | (uintptr_t)numel) & 7) ||
      (((uintptr_t)chunk_start | (uintptr_t)group | (uintptr_t)steps | (uintptr_t)scalars) & 3) ||
      (grad_scale && ((uintptr_t)grad_scale & 3)) || (found_inf && ((uintptr_t)found_inf & 3)))
    return SR_ERR_INVALID_ARGUMENT;
  Groups groups = {};
  for (int i = 0; i < num_groups; ++i) {
    const double* q = groups_host + (size_t)i * SR_ADAMW_GROUP_DOUBLES;
    const double lr = q[0], beta1 = q[1], beta2 = q[2], eps = q[3], wd = q[4];
    if (!(lr >= 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0) || !(wd >= 0.0))
      return SR_ERR_INVALID_ARGUMENT;
    Group& G = groups.g[i];
    G.lr = lr, G.beta1 = beta1, G.beta2 = beta2;
    G.decay = (float)(1.0 - lr * wd);
    G.w1 = (float)(1.0 - beta1);
    G.beta2f = (float)beta2;
    G.w2 = (float)(1.0 - beta2);
    G.eps = (float)eps;
  }
  Tables tb;
  tb.p = (const uint64_t*)p_ptrs, tb.g = (const uint64_t*)g_ptrs, tb.m = (const uint64_t*)m_ptrs, tb.v = (const uint64_t*)v_ptrs;
  tb.numel = numel, tb.chunk_start = chunk_start, tb.group = group, tb.steps = steps, tb.scalars = scalars;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sr_adamw_prologue_kernel, dim3((num_tensors + kT - 1) / kT), dim3(kT), 0, st, tb, groups, num_tensors,
                     found_inf);
  int rc = sr_hip_rc(hipGetLastError());
  if (rc != SR_OK || num_chunks == 0) return rc;
  hipLaunchKernelGGL(sr_adamw_kernel, dim3(num_chunks), dim3(kT), 0, st, tb, groups, num_tensors, grad_scale, found_inf);
  return sr_hip_rc(hipGetLastError());
}
