// sr_meshmetrics.hip -- mesh / point-cloud metrics: exact nearest neighbours on a uniform grid, area-weighted surface
// sampling and the Acc / Comp / Chamfer / Precision / Recall / F-score reduction.  gfx950 only.
//
// The rules are stated in include/simplerecon_hip.h, section "mesh metrics"; tests/mesh_metrics_oracle.py restates them
// in numpy.
//   keys        : a thread per point, fp64 cell coordinates, a hierarchical int32 key (coarse cell of 8^3 fine cells
//                 major, the fine cell within it minor), so that a fine cell, a z-run of fine cells inside one coarse
//                 cell, a coarse cell and a z-run of coarse cells are each one contiguous range of the sorted targets.
//   build       : after torch's sort of the keys, the sorted targets as float4 (x, y, z, original index) and a dense
//                 cell-start table (a thread per table entry, binary search over the sorted keys).
//   query       : a thread per query, in key-sorted query order.  Chebyshev shells of fine cells around the query's
//                 cell, r < SR_NN_FINE_SHELLS, then shells of coarse cells until the whole grid is covered.  After each
//                 shell the walk stops when the best d2 is below a lower bound of the computed d2 of every target outside
//                 the searched box (the argument is next to nn_bound()).  Every loop is bounded by the grid dimensions
//                 or N, all known before launch.
//   sampling    : fp64 face areas, a fixed-order fp64 inclusive prefix sum (chunks of kChunk faces, chunk totals
//                 scanned by one workgroup), then a thread per sample: counter-based hash, binary search, barycentric
//                 point.
//   reduction   : per-block fixed-order fp64 (sum of distances, count below threshold), one single-workgroup finalize.
// No float atomics anywhere: two runs give the same bits.
#include <math.h>

#include "sr_common.h"
#include "sr_block.h"

// every product and sum below is rounded on its own; nothing may be contracted into an FMA
#pragma clang fp contract(off)

namespace {

constexpr int kT = 256;
constexpr int kWaves = kT / SR_WAVE;
constexpr int kFine = SR_NN_FINE_SHELLS;
constexpr int kChunk = 64;                       // faces per thread in the area prefix sum
constexpr int kCoordClamp = 1 << 24;             // query cell coordinates are clamped to [-2^24, g + 2^24]

struct Grid {
  double mx, my, mz;   // grid origin (the targets' minimum)
  double h;            // fine cell edge
  int gx, gy, gz;      // fine cells per axis
  int cx, cy, cz;      // coarse cells per axis: ceil(g / 8)
};

__host__ __device__ inline int coarse_of(int g) { return (g + 7) >> 3; }

// Fine-cell coordinate of a point along one axis in fp64, t = (p - min) / h.
__device__ __forceinline__ double cell_t(float p, double m, double h) { return ((double)p - m) / h; }

__device__ __forceinline__ int clamp_cell(double t, int g) {
  const double f = floor(t);
  return f < 0.0 ? 0 : (f >= (double)(g - 1) ? g - 1 : (int)f);
}

__device__ __forceinline__ int clamp_wide(double t, int g) {
  const double f = floor(t);
  const double lo = -(double)kCoordClamp, hi = (double)g + (double)kCoordClamp;
  return (int)(f < lo ? lo : (f > hi ? hi : f));
}

__device__ __forceinline__ int fine_key(const Grid& G, int x, int y, int z) {
  const int c = ((x >> 3) * G.cy + (y >> 3)) * G.cz + (z >> 3);
  return c * 512 + (((x & 7) << 6) | ((y & 7) << 3) | (z & 7));
}

__device__ __forceinline__ int coarse_base(const Grid& G, int x, int y, int z) { return ((x * G.cy + y) * G.cz + z) * 512; }

__global__ __launch_bounds__(kT) void sr_nn_key_kernel(const float* __restrict__ pts, int64_t n, Grid G,
                                                       int32_t* __restrict__ keys) {
  for (int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x; i < n; i += (int64_t)gridDim.x * kT) {
    const int x = clamp_cell(cell_t(pts[i * 3 + 0], G.mx, G.h), G.gx);
    const int y = clamp_cell(cell_t(pts[i * 3 + 1], G.my, G.h), G.gy);
    const int z = clamp_cell(cell_t(pts[i * 3 + 2], G.mz, G.h), G.gz);
    keys[i] = fine_key(G, x, y, z);
  }
}

// sorted[j] = (x, y, z, bits of the original index) of target order[j]
__global__ __launch_bounds__(kT) void sr_nn_gather_kernel(const float* __restrict__ pts, const int64_t* __restrict__ order,
                                                          int64_t n, float4* __restrict__ sorted) {
  for (int64_t j = (int64_t)blockIdx.x * kT + threadIdx.x; j < n; j += (int64_t)gridDim.x * kT) {
    int64_t i = order[j];
    i = i < 0 ? 0 : (i >= n ? n - 1 : i);   // not a permutation: wrong results, never an out-of-bounds read
    sorted[j] = make_float4(pts[i * 3 + 0], pts[i * 3 + 1], pts[i * 3 + 2], __int_as_float((int)i));
  }
}

// start[k] = the number of sorted keys < k, for k in [0, cells]: a binary search of at most 32 steps per entry
__global__ __launch_bounds__(kT) void sr_nn_start_kernel(const int32_t* __restrict__ skeys, int64_t n, int64_t cells,
                                                         int32_t* __restrict__ start) {
  for (int64_t k = (int64_t)blockIdx.x * kT + threadIdx.x; k <= cells; k += (int64_t)gridDim.x * kT) {
    int64_t lo = 0, hi = n;   // first index with skeys[idx] >= k
    for (int it = 0; it < 32 && lo < hi; ++it) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)skeys[mid] < k) lo = mid + 1; else hi = mid;
    }
    start[k] = (int32_t)lo;
  }
}

struct QueryParams {
  const float* q;            // [M,3]
  const int64_t* order;      // [M] or null: query i of this thread is order[i]
  int64_t M;
  const float4* tgt;         // [N] sorted targets
  int64_t N;
  const int32_t* start;      // [cells + 1]
  Grid G;
  float* out_d2;             // [M] or null
  float* out_dist;           // [M] or null
  int32_t* out_index;        // [M] or null
};

// Lower bound of the computed d2 of every target outside the searched box of fine cells [lo, hi) (per axis, hi
// exclusive; a side at or beyond the grid's edge has no target behind it).  Returns +inf when the box covers the grid.
//
// Rounding argument.  A target in fine cell c has computed t = fl(fl(p - m) / h) in [c, c + 1) (or was clamped from
// just outside [0, g)), and |t_computed - t_exact| <= 2^-52 |t| <= 2^-26 for t <= 2^26 (two fp64 roundings), so its
// exact coordinate satisfies t_exact >= c - 2^-26 and t_exact <= c + 1 + 2^-26.  The query's t has the same relative
// error, <= 2^-52 |t_q|.  Any target outside the box lies, along some axis a with a finite side, at exact distance
// >= side_a * h from the query, side_a = t_q - lo_a or hi_a - t_q, less the margin 2^-20 + 2^-40 |t_q| (which covers
// both errors and the fp64 rounding of the subtraction).  Its fp32 d2 = (dx*dx + dy*dy) + dz*dz is then at least
// L^2 (1 - u)^3 >= L^2 (1 - 2^-22) with L the margin-reduced side * h and u = 2^-24: |fl(q - p)| >= |q - p| (1 - u),
// fl(dx*dx) >= dx^2 (1 - u), and adding non-negative terms never decreases a rounded sum.  The bound returned is
// L^2 (1 - 2^-18), below that by a wide margin of fp64 roundings; it is 0 when L^2 < 2^-100 (fp32 products there may
// be subnormal and lose the relative bound).  Coordinates are limited to |x| <= SR_NN_MAX_COORD, so d2 stays finite.
// The walk stops only when best < bound (strict): a target outside with an equal d2 and a smaller index cannot exist.
__device__ __forceinline__ double nn_bound(const Grid& G, const double (&tq)[3], const int (&lo)[3], const int (&hi)[3]) {
  const int g[3] = {G.gx, G.gy, G.gz};
  double side = __builtin_inf();
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double marg = 0x1p-20 + 0x1p-40 * fabs(tq[a]);
    if (lo[a] > 0) side = fmin(side, tq[a] - (double)lo[a] - marg);
    if (hi[a] < g[a]) side = fmin(side, (double)hi[a] - tq[a] - marg);
  }
  if (side == __builtin_inf()) return side;
  if (!(side > 0.0)) return 0.0;
  const double L = side * G.h;
  const double L2 = L * L;
  return L2 < 0x1p-100 ? 0.0 : L2 * (1.0 - 0x1p-18);
}

// Lower bound of the computed d2 of every target in the coarse cell whose first fine cell is lo (fine cells [lo, lo + 8)
// per axis).  The argument of nn_bound() applies per axis: the exact distance along axis a is at least gap_a * h less
// the same margin, and the fp32 d2 of a target is then at least sum_a L_a^2 (1 - u)^5 (three squares, two sums) >=
// sum_a L_a^2 (1 - 2^-21); the bound returned is that sum times (1 - 2^-18), or 0 below 2^-100.  A cell is skipped only
// when this bound is strictly greater than the best d2: none of its targets can equal or beat it.
__device__ __forceinline__ double cell_bound(const Grid& G, const double (&tq)[3], const int (&lo)[3]) {
  double s = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double marg = 0x1p-20 + 0x1p-40 * fabs(tq[a]);
    const double l = (double)lo[a], hi = (double)lo[a] + 8.0;
    double gap = tq[a] < l ? l - tq[a] : (tq[a] > hi ? tq[a] - hi : 0.0);
    gap -= marg;
    if (gap > 0.0) s += gap * gap;
  }
  const double L2 = s * (G.h * G.h);
  return L2 < 0x1p-100 ? 0.0 : L2 * (1.0 - 0x1p-18);
}

__device__ __forceinline__ void scan_range(const float4* __restrict__ tgt, int s, int e, float qx, float qy, float qz,
                                           float& best, int& bi) {
  for (int j = s; j < e; ++j) {
    const float4 t = tgt[j];
    const float dx = qx - t.x, dy = qy - t.y, dz = qz - t.z;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    const int id = __float_as_int(t.w);
    if (d2 < best || (d2 == best && id < bi)) {
      best = d2;
      bi = id;
    }
  }
}

// Chebyshev distance from integer cell c to the box [0, g) per axis
__device__ __forceinline__ int cheb_to_grid(const int (&c)[3], const int (&g)[3]) {
  int r = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const int d = c[a] < 0 ? -c[a] : (c[a] >= g[a] ? c[a] - g[a] + 1 : 0);
    r = d > r ? d : r;
  }
  return r;
}

// Visits the shell of Chebyshev radius r around cell c, clipped to [0, g), as z-runs: row(x, y, z0, z1).
template <typename Row>
__device__ __forceinline__ void visit_shell(const int (&c)[3], int r, const int (&g)[3], Row row) {
  const int x0 = max(c[0] - r, 0), x1 = min(c[0] + r, g[0] - 1);
  const int y0 = max(c[1] - r, 0), y1 = min(c[1] + r, g[1] - 1);
  const int z0 = max(c[2] - r, 0), z1 = min(c[2] + r, g[2] - 1);
  if (x0 > x1 || y0 > y1 || z0 > z1) return;   // the shell misses the grid
  const bool zlo = c[2] - r >= 0 && c[2] - r < g[2];            // the two z faces meet the grid
  const bool zhi = r > 0 && c[2] + r >= 0 && c[2] + r < g[2];
  for (int x = x0; x <= x1; ++x) {          // at most g[0] iterations
    if (x == c[0] - r || x == c[0] + r) {   // an x face: every (y, z) of the shell
      for (int y = y0; y <= y1; ++y) row(x, y, z0, z1);
      continue;
    }
    if (y0 == c[1] - r) row(x, y0, z0, z1);                // the y faces
    if (r > 0 && y1 == c[1] + r) row(x, y1, z0, z1);
    if (!zlo && !zhi) continue;                            // the z faces: single cells of the interior (x, y)
    const int ya = max(c[1] - r + 1, 0), yb = min(c[1] + r - 1, g[1] - 1);
    for (int y = ya; y <= yb; ++y) {        // at most g[1] iterations
      if (zlo) row(x, y, c[2] - r, c[2] - r);
      if (zhi) row(x, y, c[2] + r, c[2] + r);
    }
  }
}

__global__ __launch_bounds__(kT) void sr_nn_query_kernel(QueryParams p) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= p.M) return;
  int64_t qi = p.order ? p.order[i] : i;
  if (qi < 0 || qi >= p.M) return;   // not a permutation: that output is left unwritten, nothing is read out of bounds
  const Grid& G = p.G;
  const float qx = p.q[qi * 3 + 0], qy = p.q[qi * 3 + 1], qz = p.q[qi * 3 + 2];
  const double tq[3] = {cell_t(qx, G.mx, G.h), cell_t(qy, G.my, G.h), cell_t(qz, G.mz, G.h)};
  const int gf[3] = {G.gx, G.gy, G.gz};
  const int gc[3] = {G.cx, G.cy, G.cz};
  const int cq[3] = {clamp_wide(tq[0], G.gx), clamp_wide(tq[1], G.gy), clamp_wide(tq[2], G.gz)};
  float best = __builtin_inff();
  int bi = 0x7fffffff;
  bool done = false;

  // fine shells r = r0 .. kFine - 1 (r0: the first shell that meets the grid)
  const float4* __restrict__ tgt = p.tgt;
  const int32_t* __restrict__ st = p.start;
  const int rf0 = cheb_to_grid(cq, gf);
  for (int r = rf0; r < kFine && !done; ++r) {
    visit_shell(cq, r, gf, [&](int x, int y, int z0, int z1) {
      for (int z = z0; z <= z1;) {   // split at coarse-cell boundaries: at most (z1 - z0) / 8 + 2 runs
        const int ze = min(z1, z | 7);
        scan_range(tgt, st[fine_key(G, x, y, z)], st[fine_key(G, x, y, ze) + 1], qx, qy, qz, best, bi);
        z = ze + 1;
      }
    });
    const int lo[3] = {cq[0] - r, cq[1] - r, cq[2] - r};
    const int hi[3] = {cq[0] + r + 1, cq[1] + r + 1, cq[2] + r + 1};
    const double B = nn_bound(G, tq, lo, hi);
    done = B == __builtin_inf() || (double)best < B;
  }

  // coarse shells: at most max(coarse dims) + 1 of them cover the whole grid from any start
  if (!done) {
    const int cc[3] = {cq[0] >> 3, cq[1] >> 3, cq[2] >> 3};   // arithmetic shift: floor division for negatives too
    const int rc0 = cheb_to_grid(cc, gc);
    const int rmax = max(gc[0], max(gc[1], gc[2]));
    for (int k = 0; k <= rmax && !done; ++k) {
      const int r = rc0 + k;
      visit_shell(cc, r, gc, [&](int x, int y, int z0, int z1) {
        for (int z = z0; z <= z1; ++z) {   // a coarse cell is skipped when its lower bound exceeds the best d2
          const int lo[3] = {8 * x, 8 * y, 8 * z};
          if (cell_bound(G, tq, lo) > (double)best) continue;
          const int k = coarse_base(G, x, y, z);
          scan_range(tgt, st[k], st[k + 512], qx, qy, qz, best, bi);
        }
      });
      const int lo[3] = {8 * (cc[0] - r), 8 * (cc[1] - r), 8 * (cc[2] - r)};
      const int hi[3] = {8 * (cc[0] + r + 1), 8 * (cc[1] + r + 1), 8 * (cc[2] + r + 1)};
      const double B = nn_bound(G, tq, lo, hi);
      done = B == __builtin_inf() || (double)best < B;
    }
  }
  if (p.out_d2) p.out_d2[qi] = best;
  if (p.out_dist) p.out_dist[qi] = sqrtf(best);   // correctly rounded at -fno-fast-math (not __fsqrt_rn: see header)
  if (p.out_index) p.out_index[qi] = bi;
}

// ------------------------------------------------------------------------------------------------ sampling ------
__host__ __device__ inline uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ double face_area(const float* __restrict__ v, const int* __restrict__ f, int64_t V, int64_t i) {
  int ia = f[i * 3 + 0], ib = f[i * 3 + 1], ic = f[i * 3 + 2];
  if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) return 0.0;   // refused by the caller; no OOB read
  const double ax = v[ia * 3 + 0], ay = v[ia * 3 + 1], az = v[ia * 3 + 2];
  const double ux = v[ib * 3 + 0] - ax, uy = v[ib * 3 + 1] - ay, uz = v[ib * 3 + 2] - az;
  const double wx = v[ic * 3 + 0] - ax, wy = v[ic * 3 + 1] - ay, wz = v[ic * 3 + 2] - az;
  const double cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
  return 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
}

// chunk totals: a thread per chunk of kChunk faces, summed in face order
__global__ __launch_bounds__(kT) void sr_area_chunk_kernel(const float* __restrict__ v, int64_t V,
                                                           const int* __restrict__ f, int64_t F,
                                                           double* __restrict__ chunk_sum, int64_t chunks) {
  const int64_t c = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (c >= chunks) return;
  double s = 0.0;
  const int64_t e = min(F, (c + 1) * kChunk);
  for (int64_t i = c * kChunk; i < e; ++i) s += face_area(v, f, V, i);
  chunk_sum[c] = s;
}

// exclusive prefix of the chunk totals, in place, by one workgroup: thread t sums a contiguous slice sequentially, the
// slice totals are scanned sequentially by thread 0, then each thread rewrites its slice
__global__ __launch_bounds__(kT) void sr_area_scan_kernel(double* __restrict__ chunk_sum, int64_t chunks) {
  __shared__ double part[kT];
  const int64_t per = (chunks + kT - 1) / kT;
  const int64_t b = (int64_t)threadIdx.x * per, e = min(chunks, b + per);
  double s = 0.0;
  for (int64_t c = b; c < e; ++c) s += chunk_sum[c];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double run = 0.0;
    for (int t = 0; t < kT; ++t) {
      const double x = part[t];
      part[t] = run;
      run += x;
    }
  }
  __syncthreads();
  double run = part[threadIdx.x];
  for (int64_t c = b; c < e; ++c) {
    const double x = chunk_sum[c];
    chunk_sum[c] = run;
    run += x;
  }
}

// inclusive prefix of the areas: chunk offset + the chunk's areas in face order
__global__ __launch_bounds__(kT) void sr_area_prefix_kernel(const float* __restrict__ v, int64_t V,
                                                            const int* __restrict__ f, int64_t F,
                                                            const double* __restrict__ chunk_off, int64_t chunks,
                                                            double* __restrict__ cdf) {
  const int64_t c = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (c >= chunks) return;
  double run = chunk_off[c];
  const int64_t e = min(F, (c + 1) * kChunk);
  for (int64_t i = c * kChunk; i < e; ++i) {
    run += face_area(v, f, V, i);
    cdf[i] = run;
  }
}

__global__ __launch_bounds__(kT) void sr_sample_kernel(const float* __restrict__ v, int64_t V, const int* __restrict__ f,
                                                       int64_t F, const double* __restrict__ cdf, int64_t n,
                                                       uint64_t seed, float* __restrict__ out,
                                                       int32_t* __restrict__ out_face) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const uint64_t s = mix64(seed);
  const uint64_t h0 = mix64(s ^ (3ull * (uint64_t)i + 0ull));
  const uint64_t h1 = mix64(s ^ (3ull * (uint64_t)i + 1ull));
  const uint64_t h2 = mix64(s ^ (3ull * (uint64_t)i + 2ull));
  const double total = cdf[F - 1];
  const double x = (double)(h0 >> 12) * 0x1p-52 * total;   // < total: see the header
  int64_t lo = 0, hi = F - 1;                               // smallest face with cdf > x
  for (int it = 0; it < 64 && lo < hi; ++it) {
    const int64_t mid = (lo + hi) >> 1;
    if (cdf[mid] > x) hi = mid; else lo = mid + 1;
  }
  int ia = f[lo * 3 + 0], ib = f[lo * 3 + 1], ic = f[lo * 3 + 2];
  ia = min(max(ia, 0), (int)(V - 1));
  ib = min(max(ib, 0), (int)(V - 1));
  ic = min(max(ic, 0), (int)(V - 1));
  const float u = (float)(h1 >> 40) * 0x1p-24f;
  const float w = (float)(h2 >> 40) * 0x1p-24f;
  const float su = sqrtf(u);
  const float a = 1.0f - su, b = su * (1.0f - w), c = su * w;
#pragma unroll
  for (int k = 0; k < 3; ++k) out[i * 3 + k] = (a * v[ia * 3 + k] + b * v[ib * 3 + k]) + c * v[ic * 3 + k];
  if (out_face) out_face[i] = (int32_t)lo;
}

// ------------------------------------------------------------------------------------------------ reduction -----
// records: [blocks, 2] fp64 = (sum of distances, count below threshold); pred blocks first, then gt blocks
constexpr int kPerThread = 16;
constexpr int kBlockItems = kT * kPerThread;

__global__ __launch_bounds__(kT) void sr_mm_partial_kernel(const float* __restrict__ d_pred, int64_t m,
                                                           const float* __restrict__ d_gt, int64_t n, int64_t blocks_pred,
                                                           float thr, double* __restrict__ rec) {
  const int64_t blk = blockIdx.x;
  const bool is_pred = blk < blocks_pred;
  const float* d = is_pred ? d_pred : d_gt;
  const int64_t len = is_pred ? m : n;
  const int64_t b0 = (is_pred ? blk : blk - blocks_pred) * kBlockItems;
  double s = 0.0, c = 0.0;
  for (int k = 0; k < kPerThread; ++k) {
    const int64_t j = b0 + (int64_t)k * kT + threadIdx.x;
    if (j < len) {
      const float x = d[j];
      s += (double)x;
      c += x < thr ? 1.0 : 0.0;
    }
  }
  s = sr_wave_sum(s);
  c = sr_wave_sum(c);
  __shared__ double red[kWaves][2];
  const int lane = threadIdx.x & (SR_WAVE - 1), wv = threadIdx.x / SR_WAVE;
  if (lane == 0) { red[wv][0] = s; red[wv][1] = c; }
  __syncthreads();
  if (threadIdx.x < 2) {
    double t = red[0][threadIdx.x];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) t += red[k][threadIdx.x];
    rec[blk * 2 + threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(kT) void sr_mm_finalize_kernel(const double* __restrict__ rec, int64_t blocks_pred,
                                                            int64_t blocks_gt, int64_t m, int64_t n, int has_gt_dist,
                                                            double* __restrict__ out) {
  __shared__ double red[kWaves][4];
  double a[4] = {0.0, 0.0, 0.0, 0.0};   // pred sum, pred count, gt sum, gt count
  for (int64_t b = threadIdx.x; b < blocks_pred; b += kT) { a[0] += rec[b * 2]; a[1] += rec[b * 2 + 1]; }
  for (int64_t b = threadIdx.x; b < blocks_gt; b += kT) {
    a[2] += rec[(blocks_pred + b) * 2];
    a[3] += rec[(blocks_pred + b) * 2 + 1];
  }
  const int lane = threadIdx.x & (SR_WAVE - 1), wv = threadIdx.x / SR_WAVE;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double t = sr_wave_sum(a[k]);
    if (lane == 0) red[wv][k] = t;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double t[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    t[k] = red[0][k];
    for (int w = 1; w < kWaves; ++w) t[k] += red[w][k];
  }
  const double nan = __builtin_nan(""), inf = __builtin_inf();
  const double acc = m > 0 ? t[0] / (double)m : nan;
  const double prec = m > 0 ? t[1] / (double)m : nan;
  const double comp = has_gt_dist ? t[2] / (double)n : inf;
  const double rec_ = has_gt_dist ? t[3] / (double)n : 0.0;
  const double chamfer = m > 0 ? (acc + comp) / 2.0 : inf;   // an empty prediction: +inf, not NaN
  const double fs = (prec + rec_ > 0.0) ? 2.0 * prec * rec_ / (prec + rec_) : 0.0;   // NaN precision: P+R > 0 fails
  out[0] = acc;
  out[1] = comp;
  out[2] = chamfer;
  out[3] = prec;
  out[4] = rec_;
  out[5] = fs;
  out[6] = t[1];
  out[7] = t[3];
}

unsigned grid_for(int64_t items) {
  const int64_t b = (items + kT - 1) / kT;
  return (unsigned)(b < 16384 ? (b > 0 ? b : 1) : 16384);
}

bool finite_box(const double* b) {
  for (int k = 0; k < 6; ++k)
    if (!__builtin_isfinite(b[k]) || b[k] < -SR_NN_MAX_COORD || b[k] > SR_NN_MAX_COORD) return false;
  return b[0] <= b[3] && b[1] <= b[4] && b[2] <= b[5];
}

int64_t padded_cells(const int (&g)[3]) {
  return (int64_t)512 * coarse_of(g[0]) * coarse_of(g[1]) * coarse_of(g[2]);
}

bool grid_ok(double mx, double my, double mz, double h, int gx, int gy, int gz) {
  if (!__builtin_isfinite(mx) || !__builtin_isfinite(my) || !__builtin_isfinite(mz)) return false;
  if (!(h > 0.0) || !__builtin_isfinite(h)) return false;
  if (gx < 1 || gy < 1 || gz < 1) return false;
  const int g[3] = {gx, gy, gz};
  return padded_cells(g) <= (int64_t)SR_NN_MAX_CELLS;
}

Grid make_grid(double mx, double my, double mz, double h, int gx, int gy, int gz) {
  Grid G;
  G.mx = mx; G.my = my; G.mz = mz; G.h = h;
  G.gx = gx; G.gy = gy; G.gz = gz;
  G.cx = coarse_of(gx); G.cy = coarse_of(gy); G.cz = coarse_of(gz);
  return G;
}

}  // namespace

// ====================================================================================================================
extern "C" int sr_nn_grid_plan(int64_t n_targets, const double* target_box, int64_t max_cells, double* cell,
                               int* dims, int64_t* table_entries) {
  if (!target_box || !cell || !dims || !table_entries) return SR_ERR_INVALID_ARGUMENT;
  if (n_targets < 1 || n_targets >= ((int64_t)1 << 31)) return SR_ERR_INVALID_ARGUMENT;
  if (max_cells < 512 || max_cells > SR_NN_MAX_CELLS) return SR_ERR_INVALID_ARGUMENT;
  if (!finite_box(target_box)) return SR_ERR_INVALID_ARGUMENT;
  const double e[3] = {target_box[3] - target_box[0], target_box[4] - target_box[1], target_box[5] - target_box[2]};
  const double E = fmax(e[0], fmax(e[1], e[2]));
  double h = E > 0.0 ? E : 1.0;
  int g[3];
  auto fit = [&]() {
    for (int a = 0; a < 3; ++a) {
      const double c = floor(e[a] / h) + 1.0;
      g[a] = c > (double)(1 << 28) ? (1 << 28) : (int)c;
    }
  };
  fit();
  if (E > 0.0) {
    for (int k = 0; k < 200 && (double)g[0] * g[1] * g[2] < (double)n_targets; ++k) {
      h *= 0.8;
      fit();
    }
    for (int k = 0; k < 200 && padded_cells(g) > max_cells; ++k) {
      h *= 1.25;
      fit();
    }
  }
  if (padded_cells(g) > max_cells) return SR_ERR_UNSUPPORTED;
  *cell = h;
  dims[0] = g[0]; dims[1] = g[1]; dims[2] = g[2];
  *table_entries = padded_cells(g) + 1;
  return SR_OK;
}

extern "C" int sr_nn_keys(const float* points, int64_t n, double min_x, double min_y, double min_z, double cell, int gx,
                          int gy, int gz, int32_t* keys, void* stream) {
  if (n < 0 || n >= ((int64_t)1 << 31) || (n > 0 && (!points || !keys))) return SR_ERR_INVALID_ARGUMENT;
  if (!grid_ok(min_x, min_y, min_z, cell, gx, gy, gz)) return SR_ERR_INVALID_ARGUMENT;
  if (n == 0) return SR_OK;
  const Grid G = make_grid(min_x, min_y, min_z, cell, gx, gy, gz);
  hipLaunchKernelGGL(sr_nn_key_kernel, dim3(grid_for(n)), dim3(kT), 0, (hipStream_t)stream, points, n, G, keys);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_nn_build(const float* targets, int64_t n, const int32_t* sorted_keys, const int64_t* order,
                           int64_t table_entries, float* sorted_targets, int32_t* cell_start, void* stream) {
  if (n < 1 || n >= ((int64_t)1 << 31)) return SR_ERR_INVALID_ARGUMENT;
  if (!targets || !sorted_keys || !order || !sorted_targets || !cell_start) return SR_ERR_INVALID_ARGUMENT;
  if (table_entries < 513 || table_entries > (int64_t)SR_NN_MAX_CELLS + 1) return SR_ERR_INVALID_ARGUMENT;
  if ((uintptr_t)sorted_targets % 16) return SR_ERR_INVALID_ARGUMENT;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sr_nn_gather_kernel, dim3(grid_for(n)), dim3(kT), 0, st, targets, order, n,
                     (float4*)sorted_targets);
  int rc = sr_hip_rc(hipGetLastError());
  if (rc) return rc;
  hipLaunchKernelGGL(sr_nn_start_kernel, dim3(grid_for(table_entries)), dim3(kT), 0, st, sorted_keys, n,
                     table_entries - 1, cell_start);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_nn_query(const float* queries, int64_t m, const int64_t* query_order, const float* sorted_targets,
                           int64_t n, const int32_t* cell_start, int64_t table_entries, double min_x, double min_y,
                           double min_z, double cell, int gx, int gy, int gz, float* out_d2, float* out_dist,
                           int32_t* out_index, void* stream) {
  if (m < 0 || m >= ((int64_t)1 << 31) || n < 1 || n >= ((int64_t)1 << 31)) return SR_ERR_INVALID_ARGUMENT;
  if (!sorted_targets || !cell_start) return SR_ERR_INVALID_ARGUMENT;
  if (m > 0 && !queries) return SR_ERR_INVALID_ARGUMENT;
  if ((uintptr_t)sorted_targets % 16) return SR_ERR_INVALID_ARGUMENT;
  if (!grid_ok(min_x, min_y, min_z, cell, gx, gy, gz)) return SR_ERR_INVALID_ARGUMENT;
  const Grid G = make_grid(min_x, min_y, min_z, cell, gx, gy, gz);
  const int g[3] = {gx, gy, gz};
  if (table_entries != padded_cells(g) + 1) return SR_ERR_INVALID_ARGUMENT;
  if (m == 0) return SR_OK;
  QueryParams P;
  P.q = queries; P.order = query_order; P.M = m;
  P.tgt = (const float4*)sorted_targets; P.N = n;
  P.start = cell_start;
  P.G = G;
  P.out_d2 = out_d2; P.out_dist = out_dist; P.out_index = out_index;
  const unsigned blocks = (unsigned)((m + kT - 1) / kT);
  hipLaunchKernelGGL(sr_nn_query_kernel, dim3(blocks), dim3(kT), 0, (hipStream_t)stream, P);
  return sr_hip_rc(hipGetLastError());
}

extern "C" size_t sr_sample_surface_workspace_bytes(int64_t num_faces) {
  if (num_faces < 1 || num_faces >= ((int64_t)1 << 31)) return 0;
  const int64_t chunks = (num_faces + kChunk - 1) / kChunk;
  return (size_t)chunks * sizeof(double);
}

extern "C" int sr_sample_surface_cdf(const float* vertices, int64_t num_vertices, const int32_t* faces, int64_t num_faces,
                                     double* cdf, void* scratch, size_t scratch_bytes, void* stream) {
  if (!vertices || !faces || !cdf || !scratch) return SR_ERR_INVALID_ARGUMENT;
  if (num_vertices < 1 || num_vertices >= ((int64_t)1 << 31)) return SR_ERR_INVALID_ARGUMENT;
  if (num_faces < 1 || num_faces >= ((int64_t)1 << 31)) return SR_ERR_INVALID_ARGUMENT;
  if (scratch_bytes < (size_t)((num_faces + kChunk - 1) / kChunk) * sizeof(double)) return SR_ERR_WORKSPACE_TOO_SMALL;
  if ((uintptr_t)scratch % 8 || (uintptr_t)cdf % 8) return SR_ERR_INVALID_ARGUMENT;
  const int64_t chunks = (num_faces + kChunk - 1) / kChunk;
  double* csum = (double*)scratch;
  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = (unsigned)((chunks + kT - 1) / kT);
  hipLaunchKernelGGL(sr_area_chunk_kernel, dim3(blocks), dim3(kT), 0, st, vertices, num_vertices, faces, num_faces,
                     csum, chunks);
  int rc = sr_hip_rc(hipGetLastError());
  if (rc) return rc;
  hipLaunchKernelGGL(sr_area_scan_kernel, dim3(1), dim3(kT), 0, st, csum, chunks);
  rc = sr_hip_rc(hipGetLastError());
  if (rc) return rc;
  hipLaunchKernelGGL(sr_area_prefix_kernel, dim3(blocks), dim3(kT), 0, st, vertices, num_vertices, faces, num_faces,
                     csum, chunks, cdf);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_sample_surface(const float* vertices, int64_t num_vertices, const int32_t* faces, int64_t num_faces,
                                 const double* cdf, int64_t n, uint64_t seed, float* out_points, int32_t* out_face,
                                 void* stream) {
  if (!vertices || !faces || !cdf) return SR_ERR_INVALID_ARGUMENT;
  if (num_vertices < 1 || num_vertices >= ((int64_t)1 << 31)) return SR_ERR_INVALID_ARGUMENT;
  if (num_faces < 1 || num_faces >= ((int64_t)1 << 31)) return SR_ERR_INVALID_ARGUMENT;
  if (n < 0 || n >= ((int64_t)1 << 31) || (n > 0 && !out_points)) return SR_ERR_INVALID_ARGUMENT;
  if (n == 0) return SR_OK;
  hipLaunchKernelGGL(sr_sample_kernel, dim3((unsigned)((n + kT - 1) / kT)), dim3(kT), 0, (hipStream_t)stream, vertices,
                     num_vertices, faces, num_faces, cdf, n, seed, out_points, out_face);
  return sr_hip_rc(hipGetLastError());
}

extern "C" size_t sr_mesh_metrics_workspace_bytes(int64_t m, int64_t n) {
  if (m < 0 || n < 1 || m >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31)) return 0;
  const int64_t b = (m + kBlockItems - 1) / kBlockItems + (n + kBlockItems - 1) / kBlockItems;
  return (size_t)(b > 0 ? b : 1) * 2 * sizeof(double);
}

extern "C" int sr_mesh_metrics(const float* dist_pred_to_gt, int64_t m, const float* dist_gt_to_pred, int64_t n,
                               float threshold, double* out, void* scratch, size_t scratch_bytes, void* stream) {
  if (!out || !scratch) return SR_ERR_INVALID_ARGUMENT;
  if (m < 0 || n < 1 || m >= ((int64_t)1 << 31) || n >= ((int64_t)1 << 31)) return SR_ERR_INVALID_ARGUMENT;
  if (m > 0 && (!dist_pred_to_gt || !dist_gt_to_pred)) return SR_ERR_INVALID_ARGUMENT;
  if (!(threshold > 0.0f) || !__builtin_isfinite(threshold)) return SR_ERR_INVALID_ARGUMENT;
  if (scratch_bytes < sr_mesh_metrics_workspace_bytes(m, n)) return SR_ERR_WORKSPACE_TOO_SMALL;
  if ((uintptr_t)scratch % 8) return SR_ERR_INVALID_ARGUMENT;
  const int64_t bp = (m + kBlockItems - 1) / kBlockItems;
  const int64_t bg = m > 0 ? (n + kBlockItems - 1) / kBlockItems : 0;   // no prediction: no gt->pred distances
  double* rec = (double*)scratch;
  hipStream_t st = (hipStream_t)stream;
  if (bp + bg > 0) {
    hipLaunchKernelGGL(sr_mm_partial_kernel, dim3((unsigned)(bp + bg)), dim3(kT), 0, st, dist_pred_to_gt, m,
                       dist_gt_to_pred, n, bp, threshold, rec);
    const int rc = sr_hip_rc(hipGetLastError());
    if (rc) return rc;
  }
  hipLaunchKernelGGL(sr_mm_finalize_kernel, dim3(1), dim3(kT), 0, st, rec, bp, bg, m, n, m > 0 ? 1 : 0, out);
  return sr_hip_rc(hipGetLastError());
}
