// sr_raster.hip -- depth / face-id rasteriser of a triangle mesh into B pinhole views (gfx950).
// Rules: include/simplerecon_hip.h, section "mesh rasteriser"; tests/raster_oracle.py is the float64 ray caster it is
// checked against.
//
// Geometry (camera transform, near clip, projection, edge functions) runs in fp64: the MI355X issues fp64 vector
// arithmetic at half the fp32 rate, setup is a few hundred instructions per (view, face) and a pixel test is twelve
// (measured: 16M pairs of a 2M-face mesh in 0.30 ms, atomics included), and the projected edges then sit
// where a float64 ray caster puts them (no sub-pixel snapping, no fp32 projection error).  Depth is the fp32 quotient c / (n . ray) of the camera-space
// plane.  The image is a buffer of 64-bit keys (depth bits << 32 | face id) under atomicMin, as the argmax keys of
// sr_dot_volume_lds.hip: the result does not depend on launch order, and equal depths go to the lowest face id.
#include "sr_common.h"

namespace {

constexpr int kT = 256;
constexpr int kSmallMaxPixels = 256;   // bounding boxes up to this many pixels are walked by one lane
constexpr int kTileW = 16, kTileH = 4; // a large triangle's box is cut into wave-sized tiles
constexpr unsigned long long kEmpty = ~0ull;

struct View {
  double r[9], t[3];       // cam_T_world rows 0..2
  double fx, fy, cxs, cys; // cxs = cx - pixel_offset: pixel centres are the integers of the shifted frame
};

struct Tri {
  double x[3], y[3];   // projected vertices, shifted frame
  float nx, ny, nz, c; // unit normal and plane constant in the camera frame: n . X = c
  int bx0, by0, bx1, by1;
};

// Layout of one large-triangle record (SR_RASTER_RECORD_BYTES).
struct Rec {
  double x[3], y[3];
  float nx, ny, nz, c;
  int32_t view, face;
  uint32_t lo, hi;   // (by0 << 16 | bx0), (by1 << 16 | bx1)
};
static_assert(sizeof(Rec) == SR_RASTER_RECORD_BYTES, "record layout");

// One edge in canonical form: the value depends on the two end points only, not on which triangle asks or in which
// direction it walks the edge, so the two triangles on a shared edge see exactly opposite signs -- no pixel is missed by
// both.  A pixel on the edge (value 0) belongs to both, which a depth image cannot show.
struct Edge {
  double lx, ly, dx, dy, s;
};

__device__ __forceinline__ Edge make_edge(double ax, double ay, double bx, double by) {
#pragma clang fp contract(off)
  // reference end: the one nearer the image origin (the difference to a pixel is then the more exact), ties by x, then y
  const double ma = fabs(ax) + fabs(ay), mb = fabs(bx) + fabs(by);
  const bool a_first = (ma < mb) || (ma == mb && (ax < bx || (ax == bx && ay <= by)));
  Edge e;
  e.lx = a_first ? ax : bx;
  e.ly = a_first ? ay : by;
  e.dx = (a_first ? bx : ax) - e.lx;
  e.dy = (a_first ? by : ay) - e.ly;
  e.s = a_first ? 1.0 : -1.0;
  return e;
}

__device__ __forceinline__ double edge_value(const Edge& e, double px, double py) {
#pragma clang fp contract(off)
  return e.dx * (py - e.ly) - e.dy * (px - e.lx);
}

// The three edges with their signs folded so that "inside or on" is value * s >= 0; false for a projected area of zero.
__device__ __forceinline__ bool make_edges(const double (&x)[3], const double (&y)[3], Edge (&e)[3]) {
  e[0] = make_edge(x[0], y[0], x[1], y[1]);
  e[1] = make_edge(x[1], y[1], x[2], y[2]);
  e[2] = make_edge(x[2], y[2], x[0], y[0]);
  const double area = edge_value(e[0], x[2], y[2]) * e[0].s;
  if (!(area != 0.0)) return false;   // (NaN fails too)
  const double o = area > 0.0 ? 1.0 : -1.0;
  e[0].s *= o;
  e[1].s *= o;
  e[2].s *= o;
  return true;
}

__device__ __forceinline__ bool covered(const Edge (&e)[3], double px, double py) {
  return (edge_value(e[0], px, py) * e[0].s >= 0.0) & (edge_value(e[1], px, py) * e[1].s >= 0.0) &
         (edge_value(e[2], px, py) * e[2].s >= 0.0);
}

__device__ __forceinline__ View load_view(const float* __restrict__ K, const float* __restrict__ T, int b, float off) {
  View v;
  const float* t = T + (int64_t)b * 16;
  const float* k = K + (int64_t)b * 16;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    v.r[3 * i + 0] = t[4 * i + 0];
    v.r[3 * i + 1] = t[4 * i + 1];
    v.r[3 * i + 2] = t[4 * i + 2];
    v.t[i] = t[4 * i + 3];
  }
  v.fx = k[0];
  v.fy = k[5];
  v.cxs = (double)k[2] - (double)off;
  v.cys = (double)k[6] - (double)off;
  return v;
}

struct P3 {
  double x, y, z;
};

__device__ __forceinline__ P3 to_camera(const View& v, const float* __restrict__ p) {
#pragma clang fp contract(off)
  const double x = p[0], y = p[1], z = p[2];
  P3 q;
  q.x = ((v.r[0] * x + v.r[1] * y) + v.r[2] * z) + v.t[0];
  q.y = ((v.r[3] * x + v.r[4] * y) + v.r[5] * z) + v.t[1];
  q.z = ((v.r[6] * x + v.r[7] * y) + v.r[8] * z) + v.t[2];
  return q;
}

// Intersection of the segment from a (in front of the clip plane) to b (behind it) with z = zc.  Always taken from the
// front vertex to the back one: both triangles on a shared edge get the same point.
__device__ __forceinline__ P3 clip_point(const P3& a, const P3& b, double zc) {
#pragma clang fp contract(off)
  const double t = (a.z - zc) / (a.z - b.z);
  P3 q;
  q.x = a.x + t * (b.x - a.x);
  q.y = a.y + t * (b.y - a.y);
  q.z = zc;
  return q;
}

// Projects the camera-space triangle and boxes it; false when the box holds no pixel centre.
__device__ __forceinline__ bool project_tri(const View& v, const P3& a, const P3& b, const P3& c, int H, int W, Tri& t) {
#pragma clang fp contract(off)
  const P3 p[3] = {a, b, c};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    t.x[i] = (v.fx * p[i].x) / p[i].z + v.cxs;
    t.y[i] = (v.fy * p[i].y) / p[i].z + v.cys;
  }
  const double x0 = fmax(ceil(fmin(fmin(t.x[0], t.x[1]), t.x[2])), 0.0);
  const double x1 = fmin(floor(fmax(fmax(t.x[0], t.x[1]), t.x[2])), (double)(W - 1));
  const double y0 = fmax(ceil(fmin(fmin(t.y[0], t.y[1]), t.y[2])), 0.0);
  const double y1 = fmin(floor(fmax(fmax(t.y[0], t.y[1]), t.y[2])), (double)(H - 1));
  const bool finite = (t.x[0] - t.x[0] == 0.0) & (t.x[1] - t.x[1] == 0.0) & (t.x[2] - t.x[2] == 0.0) &
                      (t.y[0] - t.y[0] == 0.0) & (t.y[1] - t.y[1] == 0.0) & (t.y[2] - t.y[2] == 0.0);
  if (!finite || !(x0 <= x1) || !(y0 <= y1)) return false;
  t.bx0 = (int)x0;
  t.bx1 = (int)x1;
  t.by0 = (int)y0;
  t.by1 = (int)y1;
  return true;
}

// (static indices: a run-time index would put the pair into scratch memory)
__device__ __forceinline__ void push_tri(Tri (&out)[2], int& n, const Tri& t) {
  if (n == 0) out[0] = t; else out[1] = t;
  ++n;
}

// Setup of one (view, face): the up to two projected triangles left after the near clip.  Returns their number.
__device__ __forceinline__ int setup_face(const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces,
                                          int64_t f, const View& v, int H, int W, float znear, int cull, Tri (&out)[2]) {
#pragma clang fp contract(off)
  const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) return 0;
  P3 a = to_camera(v, verts + 3 * i0), b = to_camera(v, verts + 3 * i1), c = to_camera(v, verts + 3 * i2);
  // plane: n = (b - a) x (c - a), front-facing when n points at the camera centre, i.e. n . a < 0
  const double ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z;
  const double wx = c.x - a.x, wy = c.y - a.y, wz = c.z - a.z;
  double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
  const double len2 = (nx * nx + ny * ny) + nz * nz;
  if (!(len2 > 0.0) || !(len2 < 1e300)) return 0;   // zero area, NaN or infinite vertices
  const double inv = 1.0 / sqrt(len2);
  nx *= inv;
  ny *= inv;
  nz *= inv;
  const double pc = (nx * a.x + ny * a.y) + nz * a.z;
  if (!(pc != 0.0) || (cull == SR_RASTER_CULL_BACK && !(pc < 0.0))) return 0;   // edge-on, or facing away
  // near clip at half of znear: the pixel test z >= znear decides the cut, the clip only keeps the projection finite
  const double zc = 0.5 * (double)znear;
  const bool ia = a.z > zc, ib = b.z > zc, ic = c.z > zc;
  const int n_in = (int)ia + (int)ib + (int)ic;
  if (n_in == 0) return 0;
  int n = 0;
  Tri t;
  t.nx = (float)nx;
  t.ny = (float)ny;
  t.nz = (float)nz;
  t.c = (float)pc;
  if (n_in == 3) {
    if (project_tri(v, a, b, c, H, W, t)) push_tri(out, n, t);
    return n;
  }
  // rotate (a, b, c), keeping the winding, so that the odd vertex comes first
  const bool odd_in = n_in == 1;
  if ((odd_in ? ib : !ib)) {
    const P3 s = a;
    a = b;
    b = c;
    c = s;
  } else if ((odd_in ? ic : !ic)) {
    const P3 s = c;
    c = b;
    b = a;
    a = s;
  }
  if (odd_in) {   // a in front: (a, ab, ac)
    const P3 ab = clip_point(a, b, zc), ac = clip_point(a, c, zc);
    if (project_tri(v, a, ab, ac, H, W, t)) push_tri(out, n, t);
  } else {        // a behind: the quad (ab, b, c, ca) as (b, c, ca) and (b, ca, ba)
    const P3 ba = clip_point(b, a, zc), ca = clip_point(c, a, zc);
    if (project_tri(v, b, c, ca, H, W, t)) push_tri(out, n, t);
    if (project_tri(v, b, ca, ba, H, W, t)) push_tri(out, n, t);
  }
  return n;
}

struct Shade {   // what turns a covered pixel into a key
  float ifx, ify, cxs, cys, znear;
};

__device__ __forceinline__ Shade make_shade(const View& v, float znear) {
  Shade s;
  s.ifx = (float)(1.0 / v.fx);
  s.ify = (float)(1.0 / v.fy);
  s.cxs = (float)v.cxs;
  s.cys = (float)v.cys;
  s.znear = znear;
  return s;
}

__device__ __forceinline__ void put_pixel(const Shade& s, float nx, float ny, float nz, float c, int x, int y, int face,
                                          unsigned long long* __restrict__ keys) {
#pragma clang fp contract(off)
  const float rx = ((float)x - s.cxs) * s.ifx, ry = ((float)y - s.cys) * s.ify;
  const float z = c / ((nx * rx + ny * ry) + nz);
  if (!(z >= s.znear) || !(z < __builtin_inff())) return;
  const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)face;
  if (key < *keys) atomicMin(keys, key);   // (a stale read is only ever too high: the atomic decides)
}

// Number of true `want` flags in the wave, added to *counter by one lane; returns the caller's slot.  Every lane of the
// wave must call it.
__device__ __forceinline__ int wave_take(int* counter, bool want) {
  const unsigned long long m = __ballot(want);
  if (m == 0) return -1;
  const int lane = (int)__lane_id();
  const int leader = __ffsll((long long)m) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(counter, __popcll(m));
  base = __shfl(base, leader);
  return base + __popcll(m & ((1ull << lane) - 1ull));
}

__global__ void __launch_bounds__(kT) sr_raster_fill_kernel(unsigned long long* __restrict__ keys, int64_t n,
                                                            int32_t* __restrict__ counters) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i < n) keys[i] = kEmpty;
  if (i < 2) counters[i] = 0;
}

// One thread per (view, face).  EMIT = false: small triangles are drawn, large ones counted in counters[0].
// EMIT = true: large triangles take a slot from counters[1] and leave their record and tile count.
template <bool EMIT>
__global__ void __launch_bounds__(kT) sr_raster_setup_kernel(
    const float* __restrict__ verts, int64_t V, const int32_t* __restrict__ faces, int64_t F, const float* __restrict__ K,
    const float* __restrict__ T, int B, int H, int W, float znear, float off, int cull,
    unsigned long long* __restrict__ keys, int32_t* __restrict__ counters, int64_t capacity, Rec* __restrict__ recs,
    int32_t* __restrict__ tile_counts) {
  const int64_t idx = (int64_t)blockIdx.x * kT + threadIdx.x;
  const bool valid = idx < (int64_t)B * F;
  const int b = valid ? (int)(idx / F) : 0;
  const int64_t f = valid ? idx % F : 0;
  Tri tri[2];
  int n = 0;
  View v;
  if (valid) {
    v = load_view(K, T, b, off);
    n = setup_face(verts, V, faces, f, v, H, W, znear, cull, tri);
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const Tri& t = tri[s];
    bool large = false;
    if (s < n) {
      const int bw = t.bx1 - t.bx0 + 1, bh = t.by1 - t.by0 + 1;
      large = (int64_t)bw * bh > kSmallMaxPixels;
      if (!EMIT && !large) {
        Edge e[3];
        if (make_edges(t.x, t.y, e)) {
          const Shade sh = make_shade(v, znear);
          unsigned long long* img = keys + (int64_t)b * H * W;
          for (int y = t.by0; y <= t.by1; ++y)
            for (int x = t.bx0; x <= t.bx1; ++x)
              if (covered(e, (double)x, (double)y)) put_pixel(sh, t.nx, t.ny, t.nz, t.c, x, y, (int)f, img + (int64_t)y * W + x);
        }
      }
    }
    if (!EMIT) {
      wave_take(counters, large);
    } else {
      const int slot = wave_take(counters + 1, large);
      if (large && slot < capacity) {
        Rec r;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          r.x[i] = t.x[i];
          r.y[i] = t.y[i];
        }
        r.nx = t.nx;
        r.ny = t.ny;
        r.nz = t.nz;
        r.c = t.c;
        r.view = b;
        r.face = (int32_t)f;
        r.lo = ((uint32_t)t.by0 << 16) | (uint32_t)t.bx0;
        r.hi = ((uint32_t)t.by1 << 16) | (uint32_t)t.bx1;
        recs[slot] = r;
        const int tx = (t.bx1 - t.bx0) / kTileW + 1, ty = (t.by1 - t.by0) / kTileH + 1;
        tile_counts[slot] = tx * ty;
      }
    }
  }
}

// One wave per (large triangle, tile): the item's triangle by binary search in the inclusive prefix sums of the tile
// counts, one lane per pixel of the tile.
__global__ void __launch_bounds__(kT) sr_raster_large_kernel(const Rec* __restrict__ recs,
                                                             const int64_t* __restrict__ tile_ends, int64_t n_large,
                                                             int64_t n_items, const float* __restrict__ K, int B, int H,
                                                             int W, float znear, float off,
                                                             unsigned long long* __restrict__ keys) {
  const int64_t item = (int64_t)blockIdx.x * (kT / SR_WAVE) + (threadIdx.x / SR_WAVE);
  if (item >= n_items) return;
  int64_t lo = 0, hi = n_large - 1;   // first record with tile_ends > item
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (tile_ends[mid] > item) hi = mid; else lo = mid + 1;
  }
  const Rec r = recs[lo];
  const int64_t local = item - (lo ? tile_ends[lo - 1] : 0);
  const int bx0 = (int)(r.lo & 0xffffu), by0 = (int)(r.lo >> 16), bx1 = (int)(r.hi & 0xffffu), by1 = (int)(r.hi >> 16);
  const int tiles_x = (bx1 - bx0) / kTileW + 1;
  const int lane = threadIdx.x % SR_WAVE;
  const int x = bx0 + (int)(local % tiles_x) * kTileW + (lane % kTileW);
  const int y = by0 + (int)(local / tiles_x) * kTileH + (lane / kTileW);
  if (x > bx1 || y > by1 || x >= W || y >= H || r.view < 0 || r.view >= B) return;
  Edge e[3];
  if (!make_edges(r.x, r.y, e)) return;
  if (!covered(e, (double)x, (double)y)) return;
  const float* k = K + (int64_t)r.view * 16;
  Shade sh;
  sh.ifx = (float)(1.0 / (double)k[0]);
  sh.ify = (float)(1.0 / (double)k[5]);
  sh.cxs = (float)((double)k[2] - (double)off);
  sh.cys = (float)((double)k[6] - (double)off);
  sh.znear = znear;
  put_pixel(sh, r.nx, r.ny, r.nz, r.c, x, y, r.face, keys + ((int64_t)r.view * H + y) * W + x);
}

__global__ void __launch_bounds__(kT) sr_raster_resolve_kernel(const unsigned long long* __restrict__ keys, int64_t n,
                                                               float* __restrict__ depth, int32_t* __restrict__ face) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = keys[i];
  const bool hit = k != kEmpty;
  if (depth) depth[i] = hit ? __uint_as_float((unsigned)(k >> 32)) : 0.0f;
  if (face) face[i] = hit ? (int32_t)(unsigned)(k & 0xffffffffull) : -1;
}

__global__ void __launch_bounds__(kT) sr_raster_vis_mask_kernel(const int32_t* __restrict__ face, int B, int64_t HW,
                                                                int64_t F, unsigned long long* __restrict__ masks) {
  const int64_t i = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (i >= (int64_t)B * HW) return;
  const int32_t f = face[i];
  if (f < 0 || f >= F) return;
  const unsigned long long bit = 1ull << (int)(i / HW);
  if (!(masks[f] & bit)) atomicOr(masks + f, bit);
}

__global__ void __launch_bounds__(kT) sr_raster_vis_count_kernel(unsigned long long* __restrict__ masks, int64_t F,
                                                                 int32_t* __restrict__ counts, int min_views,
                                                                 uint8_t* __restrict__ visible) {
  const int64_t f = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (f >= F) return;
  const int c = counts[f] + __popcll(masks[f]);
  counts[f] = c;
  masks[f] = 0;
  if (visible) visible[f] = c >= min_views ? 1 : 0;
}

bool grid_for(int64_t n, unsigned& blocks) {
  const int64_t g = (n + kT - 1) / kT;
  if (g < 1 || g * kT > SR_RASTER_MAX_THREADS) return false;   // (a launch holds fewer than 2^32 threads)
  blocks = (unsigned)g;
  return true;
}

bool scene_ok(const float* verts, int64_t V, const int32_t* faces, int64_t F, const float* K, const float* T, int B, int H,
              int W, float znear, float off, int cull) {
  if (!verts || !faces || !K || !T) return false;
  if (V < 1 || V >= ((int64_t)1 << 31) || F < 1 || F >= ((int64_t)1 << 31)) return false;
  if (B < 1 || H < 1 || W < 1 || H > SR_RASTER_MAX_SIDE || W > SR_RASTER_MAX_SIDE) return false;
  if ((int64_t)B * F > SR_RASTER_MAX_PAIRS) return false;   // two triangles per pair still count in an int32
  if (!(znear > 0.0f) || !(znear < 1e30f) || !(off >= -1.0f && off <= 1.0f)) return false;
  return cull == SR_RASTER_CULL_NONE || cull == SR_RASTER_CULL_BACK;
}

}  // namespace

extern "C" int sr_raster_small(const float* vertices, int64_t num_vertices, const int32_t* faces, int64_t num_faces,
                               const float* K, const float* cam_T_world, int B, int H, int W, float znear,
                               float pixel_offset, int cull, uint64_t* keys, int32_t* counters, void* stream) {
  if (!scene_ok(vertices, num_vertices, faces, num_faces, K, cam_T_world, B, H, W, znear, pixel_offset, cull))
    return SR_ERR_INVALID_ARGUMENT;
  if (!keys || !counters) return SR_ERR_INVALID_ARGUMENT;
  unsigned gk, gs;
  if (!grid_for((int64_t)B * H * W, gk) || !grid_for((int64_t)B * num_faces, gs)) return SR_ERR_INVALID_ARGUMENT;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sr_raster_fill_kernel, dim3(gk), dim3(kT), 0, st, (unsigned long long*)keys, (int64_t)B * H * W,
                     counters);
  int rc = sr_hip_rc(hipGetLastError());
  if (rc) return rc;
  hipLaunchKernelGGL(sr_raster_setup_kernel<false>, dim3(gs), dim3(kT), 0, st, vertices, num_vertices, faces, num_faces, K,
                     cam_T_world, B, H, W, znear, pixel_offset, cull, (unsigned long long*)keys, counters, (int64_t)0,
                     (Rec*)nullptr, (int32_t*)nullptr);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_raster_large_setup(const float* vertices, int64_t num_vertices, const int32_t* faces, int64_t num_faces,
                                     const float* K, const float* cam_T_world, int B, int H, int W, float znear,
                                     float pixel_offset, int cull, int64_t capacity, int32_t* counters, void* records,
                                     int32_t* tile_counts, void* stream) {
  if (!scene_ok(vertices, num_vertices, faces, num_faces, K, cam_T_world, B, H, W, znear, pixel_offset, cull))
    return SR_ERR_INVALID_ARGUMENT;
  if (!counters || !records || !tile_counts || capacity < 1 || ((size_t)records & 7)) return SR_ERR_INVALID_ARGUMENT;
  unsigned gs;
  if (!grid_for((int64_t)B * num_faces, gs)) return SR_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(sr_raster_setup_kernel<true>, dim3(gs), dim3(kT), 0, (hipStream_t)stream, vertices, num_vertices,
                     faces, num_faces, K, cam_T_world, B, H, W, znear, pixel_offset, cull, (unsigned long long*)nullptr,
                     counters, capacity, (Rec*)records, tile_counts);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_raster_large(const void* records, const int64_t* tile_ends, int64_t num_large, int64_t num_items,
                               const float* K, int B, int H, int W, float znear, float pixel_offset, uint64_t* keys,
                               void* stream) {
  if (!records || !tile_ends || !K || !keys || ((size_t)records & 7)) return SR_ERR_INVALID_ARGUMENT;
  if (num_large < 1 || num_items < 1 || B < 1 || H < 1 || W < 1 || H > SR_RASTER_MAX_SIDE || W > SR_RASTER_MAX_SIDE)
    return SR_ERR_INVALID_ARGUMENT;
  if (!(znear > 0.0f)) return SR_ERR_INVALID_ARGUMENT;
  const int64_t per_block = kT / SR_WAVE;
  const int64_t g = (num_items + per_block - 1) / per_block;
  if (g * kT > SR_RASTER_MAX_THREADS) return SR_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(sr_raster_large_kernel, dim3((unsigned)g), dim3(kT), 0, (hipStream_t)stream, (const Rec*)records,
                     tile_ends, num_large, num_items, K, B, H, W, znear, pixel_offset, (unsigned long long*)keys);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_raster_resolve(const uint64_t* keys, int64_t n, float* depth, int32_t* face, void* stream) {
  unsigned g;
  if (!keys || (!depth && !face) || !grid_for(n, g)) return SR_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(sr_raster_resolve_kernel, dim3(g), dim3(kT), 0, (hipStream_t)stream,
                     (const unsigned long long*)keys, n, depth, face);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_raster_visibility_mask(const int32_t* face_bhw, int B, int64_t pixels_per_view, int64_t num_faces,
                                         uint64_t* masks, void* stream) {
  unsigned g;
  if (!face_bhw || !masks || B < 1 || B > SR_RASTER_MASK_VIEWS || pixels_per_view < 1 || num_faces < 1)
    return SR_ERR_INVALID_ARGUMENT;
  if (!grid_for((int64_t)B * pixels_per_view, g)) return SR_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(sr_raster_vis_mask_kernel, dim3(g), dim3(kT), 0, (hipStream_t)stream, face_bhw, B, pixels_per_view,
                     num_faces, (unsigned long long*)masks);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_raster_visibility_count(uint64_t* masks, int64_t num_faces, int32_t* counts, int min_views,
                                          uint8_t* visible, void* stream) {
  unsigned g;
  if (!masks || !counts || min_views < 1 || !grid_for(num_faces, g)) return SR_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(sr_raster_vis_count_kernel, dim3(g), dim3(kT), 0, (hipStream_t)stream, (unsigned long long*)masks,
                     num_faces, counts, min_views, visible);
  return sr_hip_rc(hipGetLastError());
}
