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
//
// Gradient statistics (sr_grad_stats): one read-only pass over the same chunk table sums the squares of every gradient in
// double, one workgroup per chunk and one partial per workgroup, and a one-workgroup finalise launch adds the partials in
// a fixed order into per-tensor norms, the global norm, the non-finite flag, torch's clip coefficient and (optionally)
// the loss scaler's update.  sr_adamw_step_clipped multiplies that coefficient in registers; sr_grad_scale_inplace is the
// in-place multiply of torch's clip_grad_norm_.
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
  float decay, w1, beta2, w2, eps, neg_step_size, bc2_sqrt, grad_scale, grad_coef;
  bool scaled, clipped;
};

// the last tensor whose first chunk is at or in front of c (tensors without elements have none)
__device__ __forceinline__ int tensor_of_chunk(const int32_t* __restrict__ chunk_start, int T, int c) {
  int lo = 0, hi = T;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (chunk_start[mid] <= c) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ void update(float& p, float g, float& m, float& v, const Hyper& h) {
  if (h.scaled) g = g / h.grad_scale;
  if (h.clipped) g = g * h.grad_coef;
  p = p * h.decay;
  const float d = g - m;
  m = h.w1 < 0.5f ? fmaf(h.w1, d, m) : fmaf(h.w1 - 1.0f, d, g);   // lerp(m, g, 1 - beta1)
  v = v * h.beta2;
  v = fmaf(h.w2 * g, g, v);
  const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
  p = p + (h.neg_step_size * m) / denom;
}

__global__ __launch_bounds__(kT) void sr_adamw_kernel(Tables tb, Groups groups, int T, const float* grad_scale,
                                                      const float* found_inf, const float* grad_coef) {
  if (skipped(found_inf)) return;
  const int c = blockIdx.x;
  const int t = tensor_of_chunk(tb.chunk_start, T, c);
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
  h.clipped = grad_coef != nullptr;
  h.grad_coef = h.clipped ? *grad_coef : 1.0f;
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

// ---- gradient statistics -------------------------------------------------------------------------------------------------

constexpr int kWaves = kT / 64;
constexpr int kFinT = 1024;   // the finalise launch: one workgroup, one thread per tensor and round
constexpr int kFinTile = 4096; // partials it stages in LDS at a time

__device__ __forceinline__ double squared(float x) {
  const double d = (double)x;
  return d * d;
}

// One partial per chunk: the sum of squares of the chunk's elements in double, lane sums in element order, then a fixed
// tree over the wave and the four wave sums in order.  Every chunk writes its partial (0 for a tensor without a gradient).
__global__ __launch_bounds__(kT) void sr_grad_sumsq_kernel(const uint64_t* __restrict__ g_ptrs, const int64_t* __restrict__ numel,
                                                           const int32_t* __restrict__ chunk_start, int T,
                                                           double* __restrict__ partials) {
  __shared__ double wave_sum[kWaves];
  const int c = blockIdx.x;
  const int t = tensor_of_chunk(chunk_start, T, c);
  const uint64_t address = g_ptrs[t];
  const int64_t off = (int64_t)(c - chunk_start[t]) * kChunk;
  const int64_t left = numel[t] - off;
  const int cnt = address == 0 || left <= 0 ? 0 : left < kChunk ? (int)left : kChunk;
  const float* __restrict__ g = (const float*)address + off;
  double acc = 0.0;
  if ((address & 15) == 0) {   // (off is a multiple of kChunk)
    const int nvec = cnt >> 2;
    float4 G[kVecIters];
#pragma unroll
    for (int k = 0; k < kVecIters; ++k) {
      const int i = threadIdx.x + k * kT;
      G[k] = i < nvec ? ((const float4*)g)[i] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    const int i = (nvec << 2) + threadIdx.x;   // the tail of the tensor's last chunk: up to three floats
    const float tail = threadIdx.x < 3 && i < cnt ? g[i] : 0.0f;
#pragma unroll
    for (int k = 0; k < kVecIters; ++k) {
      acc += squared(G[k].x);
      acc += squared(G[k].y);
      acc += squared(G[k].z);
      acc += squared(G[k].w);
    }
    acc += squared(tail);
  } else {
#pragma unroll
    for (int k0 = 0; k0 < kIters; k0 += 4) {
      float x[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int i = threadIdx.x + (k0 + k) * kT;
        x[k] = i < cnt ? g[i] : 0.0f;
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) acc += squared(x[k]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = wave_sum[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) s += wave_sum[w];
    partials[c] = s;
  }
}

struct Scaler {
  float* scale;            // the loss scale: read as this step's scale, then updated
  int32_t* tracker;        // steps without a non-finite gradient since the last change
  double growth, backoff;
  int interval;
};

// One workgroup.  The partials of a round of kFinT tensors are consecutive: they are staged in LDS kFinTile at a time with
// coalesced loads, each thread adds its tensor's partials in chunk order out of LDS, then thread 0 adds the tensors in
// index order: no atomics, the same bytes on every run.
__global__ __launch_bounds__(kFinT) void sr_grad_finalise_kernel(const int32_t* __restrict__ chunk_start, int T,
                                                                 const double* __restrict__ partials,
                                                                 const float* grad_scale, float max_norm,
                                                                 float* __restrict__ norms, float* __restrict__ stats,
                                                                 Scaler scaler) {
  __shared__ double sums[kFinT];
  __shared__ double tile[kFinTile];
  const float scale = scaler.scale != nullptr ? *scaler.scale : grad_scale != nullptr ? *grad_scale : 1.0f;
  double total = 0.0;
  for (int base = 0; base < T; base += kFinT) {
    const int t = base + threadIdx.x;
    const int lo = chunk_start[base], hi = chunk_start[base + kFinT < T ? base + kFinT : T];   // the round's partials
    const int mine_lo = t < T ? chunk_start[t] : hi, mine_hi = t < T ? chunk_start[t + 1] : hi;
    double s = 0.0;
    for (int c0 = lo; c0 < hi; c0 += kFinTile) {
      const int n = hi - c0 < kFinTile ? hi - c0 : kFinTile;
      for (int j = threadIdx.x; j < n; j += kFinT) tile[j] = partials[c0 + j];
      __syncthreads();
      const int from = mine_lo > c0 ? mine_lo : c0, to = mine_hi < c0 + n ? mine_hi : c0 + n;
#pragma unroll 8
      for (int c = from; c < to; ++c) s += tile[c - c0];
      __syncthreads();
    }
    if (t < T) {
      sums[threadIdx.x] = s;
      norms[t] = (float)(sqrt(s) / (double)scale);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int n = T - base < kFinT ? T - base : kFinT;
#pragma unroll 8
      for (int i = 0; i < n; ++i) total += sums[i];
    }
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const float total_norm = (float)(sqrt(total) / (double)scale);
  const bool found_inf = !isfinite(total);
  float coef = 1.0f;
  if (max_norm > 0.0f) {   // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (total_norm + 1e-6), max=1), NaN kept
    const float q = max_norm / (total_norm + 1e-6f);
    coef = q > 1.0f ? 1.0f : q;
  }
  stats[SR_GRAD_STATS_NORM] = total_norm;
  stats[SR_GRAD_STATS_FOUND_INF] = found_inf ? 1.0f : 0.0f;
  stats[SR_GRAD_STATS_COEF] = coef;
  stats[SR_GRAD_STATS_SCALE] = scale;
  if (scaler.scale != nullptr) {   // torch's _amp_update_scale_
    if (found_inf) {
      *scaler.scale = (float)((double)scale * scaler.backoff);
      *scaler.tracker = 0;
    } else {
      const int successful = *scaler.tracker + 1;
      if (successful == scaler.interval) {
        const float grown = (float)((double)scale * scaler.growth);
        if (isfinite(grown)) *scaler.scale = grown;
        *scaler.tracker = 0;
      } else {
        *scaler.tracker = successful;
      }
    }
  }
}

__global__ __launch_bounds__(kT) void sr_grad_scale_kernel(const uint64_t* __restrict__ g_ptrs, const int64_t* __restrict__ numel,
                                                           const int32_t* __restrict__ chunk_start, int T,
                                                           const float* __restrict__ coef_ptr) {
  const int c = blockIdx.x;
  const int t = tensor_of_chunk(chunk_start, T, c);
  const uint64_t address = g_ptrs[t];
  if (address == 0) return;
  const int64_t off = (int64_t)(c - chunk_start[t]) * kChunk;
  const int64_t left = numel[t] - off;
  if (left <= 0) return;
  const int cnt = left < kChunk ? (int)left : kChunk;
  float* __restrict__ g = (float*)address + off;
  const float coef = *coef_ptr;
  if ((address & 15) == 0) {
    const int nvec = cnt >> 2;
    float4 G[kVecIters];
#pragma unroll
    for (int k = 0; k < kVecIters; ++k) {
      const int i = threadIdx.x + k * kT;
      if (i < nvec) G[k] = ((const float4*)g)[i];
    }
#pragma unroll
    for (int k = 0; k < kVecIters; ++k) {
      const int i = threadIdx.x + k * kT;
      if (i < nvec) {
        G[k].x *= coef, G[k].y *= coef, G[k].z *= coef, G[k].w *= coef;
        ((float4*)g)[i] = G[k];
      }
    }
    const int i = (nvec << 2) + threadIdx.x;
    if (threadIdx.x < 3 && i < cnt) g[i] *= coef;
  } else {
#pragma unroll 4
    for (int k = 0; k < kIters; ++k) {
      const int i = threadIdx.x + k * kT;
      if (i < cnt) g[i] *= coef;
    }
  }
}

// the checks the three entry points over the gradient tables share
int check_grad_tables(const void* g_ptrs, const int64_t* numel, const int32_t* chunk_start, int num_tensors, int num_chunks) {
  if (!g_ptrs || !numel || !chunk_start) return SR_ERR_INVALID_ARGUMENT;
  if (num_tensors < 1 || num_chunks < 0) return SR_ERR_INVALID_ARGUMENT;
  if (num_tensors > SR_ADAMW_MAX_TENSORS) return SR_ERR_UNSUPPORTED;
  if ((((uintptr_t)g_ptrs | (uintptr_t)numel) & 7) || ((uintptr_t)chunk_start & 3)) return SR_ERR_INVALID_ARGUMENT;
  return SR_OK;
}

}  // namespace

extern "C" int sr_adamw_step_clipped(const void* p_ptrs, const void* g_ptrs, const void* m_ptrs, const void* v_ptrs,
                                     const int64_t* numel, const int32_t* chunk_start, const int32_t* group, float* steps,
                                     float* scalars, int num_tensors, int num_chunks, const double* groups_host,
                                     int num_groups, const float* grad_scale, const float* found_inf,
                                     const float* grad_coef, void* stream) {
  if (!p_ptrs || !g_ptrs || !m_ptrs || !v_ptrs || !numel || !chunk_start || !group || !steps || !scalars || !groups_host)
    return SR_ERR_INVALID_ARGUMENT;
  if (num_tensors < 1 || num_chunks < 0 || num_groups < 1) return SR_ERR_INVALID_ARGUMENT;
  if (num_tensors > SR_ADAMW_MAX_TENSORS || num_groups > SR_ADAMW_MAX_GROUPS) return SR_ERR_UNSUPPORTED;
  if ((((uintptr_t)p_ptrs | (uintptr_t)g_ptrs | (uintptr_t)m_ptrs | (uintptr_t)v_ptrs | (uintptr_t)numel) & 7) ||
      (((uintptr_t)chunk_start | (uintptr_t)group | (uintptr_t)steps | (uintptr_t)scalars) & 3) ||
      (grad_scale && ((uintptr_t)grad_scale & 3)) || (found_inf && ((uintptr_t)found_inf & 3)) ||
      (grad_coef && ((uintptr_t)grad_coef & 3)))
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
  hipLaunchKernelGGL(sr_adamw_kernel, dim3(num_chunks), dim3(kT), 0, st, tb, groups, num_tensors, grad_scale, found_inf,
                     grad_coef);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_adamw_step(const void* p_ptrs, const void* g_ptrs, const void* m_ptrs, const void* v_ptrs,
                             const int64_t* numel, const int32_t* chunk_start, const int32_t* group, float* steps,
                             float* scalars, int num_tensors, int num_chunks, const double* groups_host, int num_groups,
                             const float* grad_scale, const float* found_inf, void* stream) {
  return sr_adamw_step_clipped(p_ptrs, g_ptrs, m_ptrs, v_ptrs, numel, chunk_start, group, steps, scalars, num_tensors,
                               num_chunks, groups_host, num_groups, grad_scale, found_inf, nullptr, stream);
}

extern "C" size_t sr_grad_stats_workspace_bytes(int num_chunks, int num_tensors) {
  (void)num_tensors;   // (per-tensor sums stay in LDS)
  return sizeof(double) * (size_t)(num_chunks > 1 ? num_chunks : 1);
}

extern "C" int sr_grad_stats(const void* g_ptrs, const int64_t* numel, const int32_t* chunk_start, int num_tensors,
                             int num_chunks, const float* grad_scale, float max_norm, float* norms, float* stats,
                             float* scaler_scale, int32_t* scaler_tracker, double growth_factor, double backoff_factor,
                             int growth_interval, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc0 = check_grad_tables(g_ptrs, numel, chunk_start, num_tensors, num_chunks);
  if (rc0 != SR_OK) return rc0;
  if (!norms || !stats || !workspace) return SR_ERR_INVALID_ARGUMENT;
  if ((((uintptr_t)norms | (uintptr_t)stats) & 3) || ((uintptr_t)workspace & 7) ||
      (grad_scale && ((uintptr_t)grad_scale & 3)) || (scaler_scale && ((uintptr_t)scaler_scale & 3)) ||
      (scaler_tracker && ((uintptr_t)scaler_tracker & 3)))
    return SR_ERR_INVALID_ARGUMENT;
  if (!(max_norm == max_norm)) return SR_ERR_INVALID_ARGUMENT;
  if ((scaler_scale == nullptr) != (scaler_tracker == nullptr) || (scaler_scale && grad_scale)) return SR_ERR_INVALID_ARGUMENT;
  if (scaler_scale && (!(growth_factor > 0.0) || !(backoff_factor > 0.0) || growth_interval < 1)) return SR_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < sr_grad_stats_workspace_bytes(num_chunks, num_tensors)) return SR_ERR_WORKSPACE_TOO_SMALL;
  const hipStream_t st = (hipStream_t)stream;
  double* partials = (double*)workspace;
  if (num_chunks > 0) {
    hipLaunchKernelGGL(sr_grad_sumsq_kernel, dim3(num_chunks), dim3(kT), 0, st, (const uint64_t*)g_ptrs, numel, chunk_start,
                       num_tensors, partials);
    const int rc = sr_hip_rc(hipGetLastError());
    if (rc != SR_OK) return rc;
  }
  Scaler scaler;
  scaler.scale = scaler_scale, scaler.tracker = scaler_tracker;
  scaler.growth = growth_factor, scaler.backoff = backoff_factor, scaler.interval = growth_interval;
  hipLaunchKernelGGL(sr_grad_finalise_kernel, dim3(1), dim3(kFinT), 0, st, chunk_start, num_tensors, partials, grad_scale,
                     max_norm, norms, stats, scaler);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_grad_scale_inplace(const void* g_ptrs, const int64_t* numel, const int32_t* chunk_start, int num_tensors,
                                     int num_chunks, const float* coef, void* stream) {
  const int rc0 = check_grad_tables(g_ptrs, numel, chunk_start, num_tensors, num_chunks);
  if (rc0 != SR_OK) return rc0;
  if (!coef || ((uintptr_t)coef & 3)) return SR_ERR_INVALID_ARGUMENT;
  if (num_chunks == 0) return SR_OK;
  hipLaunchKernelGGL(sr_grad_scale_kernel, dim3(num_chunks), dim3(kT), 0, (hipStream_t)stream, (const uint64_t*)g_ptrs, numel,
                     chunk_start, num_tensors, coef);
  return sr_hip_rc(hipGetLastError());
}
