// sr_mesh.hip -- marching cubes on the fused fp16 TSDF volume (the mesh export of reference tools/tsdf.py:128-168,
// TSDF.to_mesh / TSDF.save, which copies the volume to the host and runs skimage's marching cubes there).  gfx950 only.
//
// The surface rules (corners, vertices, face decisions, loops, fan triangulation, degenerate triangles, coordinates)
// are stated in include/simplerecon_hip.h, section "mesh extraction"; tests/mesh_oracle.py implements the same rules
// in numpy.  Work is split so that nothing but the surface needs memory:
//   count   : one streaming pass, a thread per 8-voxel z-group, a workgroup per brick of 256 groups; every brick
//             writes its active voxels, vertices and non-degenerate triangles.
//   scan    : one workgroup turns the brick totals into 64-bit exclusive offsets and the three mesh totals.
//   compact : bricks with active voxels evaluate their voxels again and write the sorted list of active voxels
//             (linear index, vertex offset, triangle offset, edge mask).
//   emit    : a thread per active voxel writes the vertices of its own edges and the triangles of its cube; the
//             vertex of an edge owned by a neighbour is found by binary search in the sorted list.
// Everything is integer counting or a fixed sequence of fp32 operations, so the output does not depend on the schedule.
#include <hip/hip_fp16.h>

#include "sr_common.h"
#include "sr_block.h"
#include "sr_mc.h"

// edge parameters, positions and the asymptotic decider are separate fp32 operations, as in the numpy rules
#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;   // threads per workgroup; a count / compact workgroup covers kThreads z-groups of 8 voxels

__device__ __forceinline__ float load_val(const __half* vol, int64_t o) { return clamp1(__half2float(vol[o])); }

struct Params {
  const __half* vol;
  int X, Y, Z;
  int groups_z;       // ceil(Z / 8)
  int64_t groups;     // X * Y * groups_z
  int64_t nbricks;
  float level;
  int* brick_cnt;     // [3][nbricks]: active voxels, vertices, triangles of each brick
  int64_t* brick_off; // [3][nbricks]: exclusive prefix sums of brick_cnt
  int64_t* totals;    // [3]
  int64_t* keys;      // [A] linear voxel index of every active voxel, ascending
  int4* meta;         // [A] {vertex offset, triangle offset, edge mask, triangles}
  int64_t A, V, F;
  float ox, oy, oz, scale;
  float* verts;
  float* normals;
  int* faces;
};

// Loads 9 values of the z-row of voxel column (i, j) from k0 (the 9th: the first voxel of the next group).
template <bool VEC>
__device__ __forceinline__ void load_row(const Params& p, int i, int j, int k0, float r[9]) {
  const int64_t base = ((int64_t)i * p.Y + j) * p.Z + k0;
  if (VEC) {
    union { uint4 q; __half h[8]; } u;
    u.q = *reinterpret_cast<const uint4*>(p.vol + base);
#pragma unroll
    for (int m = 0; m < 8; ++m) r[m] = clamp1(__half2float(u.h[m]));
  } else {
#pragma unroll
    for (int m = 0; m < 8; ++m) r[m] = k0 + m < p.Z ? load_val(p.vol, base + m) : 0.0f;
  }
  r[8] = k0 + 8 < p.Z ? load_val(p.vol, base + 8) : 0.0f;
  // positions past the end repeat the first value: they never reach a result, and keep a uniform row uniform
#pragma unroll
  for (int m = 1; m < 9; ++m)
    if (k0 + m >= p.Z) r[m] = r[0];
}

// Per thread: the 8 voxels (i, j, k0..k0+7) of one z-group; returns their (active, vertices, triangles) and, in
// `packed`, 7 bits per voxel (edge mask | triangles << 3).
template <bool VEC>
__device__ __forceinline__ void group_info(const Params& p, int64_t g, int& act, int& nv, int& nt, uint64_t& packed) {
  act = nv = nt = 0;
  packed = 0;
  if (g >= p.groups) return;
  const int64_t col = g / p.groups_z;
  const int k0 = (int)(g - col * p.groups_z) * 8;
  const int i = (int)(col / p.Y), j = (int)(col - (int64_t)i * p.Y);
  const bool hx = i + 1 < p.X, hy = j + 1 < p.Y;
  float r00[9], r01[9], r10[9], r11[9];
  load_row<VEC>(p, i, j, k0, r00);
  if (hy) load_row<VEC>(p, i, j + 1, k0, r01);
  if (hx) load_row<VEC>(p, i + 1, j, k0, r10);
  if (hx && hy) load_row<VEC>(p, i + 1, j + 1, k0, r11);
  // missing rows (volume border) repeat row (i, j): never used by a result
#pragma unroll
  for (int m = 0; m < 9; ++m) {
    if (!hy) r01[m] = r00[m];
    if (!hx) r10[m] = hy ? r01[m] : r00[m];
    if (!(hx && hy)) r11[m] = hx ? r10[m] : r01[m];
  }
  // most of a fused volume is untouched (-1) or far from the surface: one uniform side, nothing to do
  bool all_below = true, all_above = true;
#pragma unroll
  for (int m = 0; m < 9; ++m) {
    const float v[4] = {r00[m], r01[m], r10[m], r11[m]};
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      all_below &= v[u] < p.level;
      all_above &= !(v[u] < p.level) && !isnan(v[u]);
    }
  }
  if (all_below || all_above) return;
  const int n = min(8, p.Z - k0);
#pragma unroll 1
  for (int m = 0; m < n; ++m) {
    const float c[8] = {r00[0], r10[0], r01[0], r11[0], r00[1], r10[1], r01[1], r11[1]};
    int mask, ntri;
    voxel_info(c, hx, hy, k0 + m + 1 < p.Z, p.level, i, j, k0 + m, mask, ntri);
    act += (mask | ntri) != 0;
    nv += __popc(mask);
    nt += ntri;
    packed |= (uint64_t)(mask | (ntri << 3)) << (7 * m);
#pragma unroll
    for (int s = 0; s < 8; ++s) {  // shift the rows by one voxel (keeps every register index static)
      r00[s] = r00[s + 1]; r01[s] = r01[s + 1]; r10[s] = r10[s + 1]; r11[s] = r11[s + 1];
    }
  }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void sr_mesh_count_kernel(Params p) {
  const int64_t brick = blockIdx.x;
  int act, nv, nt;
  uint64_t packed;
  group_info<VEC>(p, brick * kThreads + threadIdx.x, act, nv, nt, packed);
  const int v[3] = {act, nv, nt};
  int excl[3], tot[3];
  sr_block_scan<3, kThreads>(v, excl, tot);
  if (threadIdx.x == 0) {
    p.brick_cnt[brick] = tot[0];
    p.brick_cnt[p.nbricks + brick] = tot[1];
    p.brick_cnt[2 * p.nbricks + brick] = tot[2];
  }
}

// One workgroup: 64-bit exclusive offsets of the three brick counters, in brick order, and the totals.
__global__ __launch_bounds__(1024) void sr_mesh_scan_kernel(Params p) {
  __shared__ int64_t s[1024];
  const int t = threadIdx.x;
  const int64_t chunk = (p.nbricks + 1023) / 1024;
  const int64_t b0 = min((int64_t)t * chunk, p.nbricks), b1 = min(b0 + chunk, p.nbricks);
#pragma unroll 1
  for (int c = 0; c < 3; ++c) {
    const int* cnt = p.brick_cnt + c * p.nbricks;
    int64_t sum = 0;
    for (int64_t b = b0; b < b1; ++b) sum += cnt[b];
    s[t] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
      const int64_t o = t >= d ? s[t - d] : 0;
      __syncthreads();
      s[t] += o;
      __syncthreads();
    }
    int64_t run = s[t] - sum;
    int64_t* off = p.brick_off + c * p.nbricks;
    for (int64_t b = b0; b < b1; ++b) {
      off[b] = run;
      run += cnt[b];
    }
    if (t == 1023) p.totals[c] = s[t];
    __syncthreads();
  }
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void sr_mesh_compact_kernel(Params p) {
  const int64_t brick = blockIdx.x;
  if (p.brick_cnt[brick] == 0) return;  // uniform over the workgroup
  const int64_t g = brick * kThreads + threadIdx.x;
  int act, nv, nt;
  uint64_t packed;
  group_info<VEC>(p, g, act, nv, nt, packed);
  const int v[3] = {act, nv, nt};
  int excl[3], tot[3];
  sr_block_scan<3, kThreads>(v, excl, tot);
  if (!act) return;
  int64_t a = p.brick_off[brick] + excl[0];
  int64_t vo = p.brick_off[p.nbricks + brick] + excl[1];
  int64_t to = p.brick_off[2 * p.nbricks + brick] + excl[2];
  const int64_t lin0 = g / p.groups_z * p.Z + (g % p.groups_z) * 8;
  for (int m = 0; m < 8; ++m) {
    const int info = (int)((packed >> (7 * m)) & 127), mask = info & 7, ntri = info >> 3;
    if (!info) continue;
    if (a < p.A) {  // always true for the volume that was counted
      p.keys[a] = lin0 + m;
      p.meta[a] = make_int4((int)vo, (int)to, mask, ntri);
    }
    ++a;
    vo += __popc(mask);
    to += ntri;
  }
}

// Central-difference gradient of the clamped values at voxel (x,y,z); one-sided at the border.
__device__ __forceinline__ void gradient(const Params& p, int x, int y, int z, float g[3]) {
  const int idx[3] = {x, y, z};
  const int dim[3] = {p.X, p.Y, p.Z};
  const int64_t stride[3] = {(int64_t)p.Y * p.Z, p.Z, 1};
  const int64_t o = ((int64_t)x * p.Y + y) * p.Z + z;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (idx[a] == 0) g[a] = load_val(p.vol, o + stride[a]) - load_val(p.vol, o);
    else if (idx[a] == dim[a] - 1) g[a] = load_val(p.vol, o) - load_val(p.vol, o - stride[a]);
    else g[a] = (load_val(p.vol, o + stride[a]) - load_val(p.vol, o - stride[a])) * 0.5f;
  }
}

__global__ __launch_bounds__(kThreads) void sr_mesh_emit_kernel(Params p) {
  const int64_t n = (int64_t)blockIdx.x * kThreads + threadIdx.x;
  if (n >= p.A) return;
  const int64_t lin = p.keys[n];
  const int4 me = p.meta[n];
  const int64_t yz = (int64_t)p.Y * p.Z;
  const int i = (int)(lin / yz), j = (int)((lin - (int64_t)i * yz) / p.Z), k = (int)(lin - (int64_t)i * yz - (int64_t)j * p.Z);
  const bool hx = i + 1 < p.X, hy = j + 1 < p.Y, hz = k + 1 < p.Z;
  float c[8];
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    const int dx = m & 1, dy = (m >> 1) & 1, dz = (m >> 2) & 1;
    const bool ok = (!dx || hx) && (!dy || hy) && (!dz || hz);
    c[m] = ok ? load_val(p.vol, lin + dx * yz + dy * p.Z + dz) : 0.0f;
  }
  // vertices of the voxel's own edges
  int r = 0;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    if (!((me.z >> a) & 1)) continue;
    const int64_t vi = (int64_t)me.x + r++;
    if (vi >= p.V) continue;
    const float v0 = c[0], v1 = c[1 << a];
    const float t = (p.level - v0) / (v1 - v0);
    float q[3] = {(float)i, (float)j, (float)k};
    q[a] = q[a] + t;
    p.verts[3 * vi + 0] = p.ox + q[0] * p.scale;
    p.verts[3 * vi + 1] = p.oy + q[1] * p.scale;
    p.verts[3 * vi + 2] = p.oz + q[2] * p.scale;
    if (p.normals) {
      float g0[3], g1[3], nv[3];
      gradient(p, i, j, k, g0);
      gradient(p, i + (a == 0), j + (a == 1), k + (a == 2), g1);
#pragma unroll
      for (int d = 0; d < 3; ++d) nv[d] = g0[d] + t * (g1[d] - g0[d]);
      const float len = sqrtf(nv[0] * nv[0] + nv[1] * nv[1] + nv[2] * nv[2]);
#pragma unroll
      for (int d = 0; d < 3; ++d) p.normals[3 * vi + d] = len > 0.0f ? nv[d] / len : 0.0f;
    }
  }
  if (!me.w) return;
  Cube q;
  cube_build(c, p.level, q);
  // global vertex index of every crossing cube edge: owner voxel's vertex offset + rank of the axis among the owner's
  // crossing edges; one search per owner corner (corner 7 owns no cube edge)
  int vbase[7], vmask[7];
  vbase[0] = me.x;
  vmask[0] = me.z;
#pragma unroll
  for (int oc = 1; oc < 7; ++oc) {
    uint32_t owned = 0;
#pragma unroll
    for (int e = 0; e < 12; ++e) owned |= edge_lo(e) == oc ? 1u << e : 0u;
    vbase[oc] = -1;
    vmask[oc] = 0;
    if (q.cross & owned) {
      // (found: the owner of a crossing edge is an active voxel, and it sorts after this one)
      const int64_t m = sr_find_sorted(p.keys, n + 1, p.A, lin + (oc & 1) * yz + ((oc >> 1) & 1) * p.Z + ((oc >> 2) & 1));
      if (m >= 0) {
        const int4 o = p.meta[m];
        vbase[oc] = o.x;
        vmask[oc] = o.z;
      }
    }
  }
  int gid[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) {
    const int oc = edge_lo(e);
    gid[e] = vbase[oc] < 0 ? -1 : vbase[oc] + __popc(vmask[oc] & ((1 << edge_ax(e)) - 1));
  }
  int64_t f = me.y;
  cube_triangles(q, i, j, k, [&](int a, int b, int cc) {
    if (f < p.F) {
      p.faces[3 * f + 0] = gid[a];
      p.faces[3 * f + 1] = gid[b];
      p.faces[3 * f + 2] = gid[cc];
    }
    ++f;
  });
}

bool fill_params(Params& P, const void* vol, int X, int Y, int Z, float level) {
  if (!vol || X < 2 || Y < 2 || Z < 2) return false;
  P = Params{};
  P.vol = (const __half*)vol;
  P.X = X; P.Y = Y; P.Z = Z;
  P.groups_z = (Z + 7) / 8;
  P.groups = (int64_t)X * Y * P.groups_z;
  P.nbricks = (P.groups + kThreads - 1) / kThreads;
  P.level = level;
  return true;
}

bool vec_path(const void* vol, int Z) { return Z % 8 == 0 && ((uintptr_t)vol & 15) == 0; }

size_t count_scratch_bytes(int64_t nbricks) { return sr_align_up((size_t)nbricks * 3 * sizeof(int), 16) + (size_t)nbricks * 3 * sizeof(int64_t); }

void bind_count_scratch(Params& P, void* scratch) {
  P.brick_cnt = (int*)scratch;
  P.brick_off = (int64_t*)((char*)scratch + sr_align_up((size_t)P.nbricks * 3 * sizeof(int), 16));
}

}  // namespace

extern "C" size_t sr_mesh_count_scratch_bytes(int X, int Y, int Z) {
  if (X < 2 || Y < 2 || Z < 2) return 0;
  const int64_t groups = (int64_t)X * Y * ((Z + 7) / 8);
  return count_scratch_bytes((groups + kThreads - 1) / kThreads);
}

extern "C" size_t sr_mesh_list_scratch_bytes(int64_t active) {
  if (active < 0) return 0;
  return sr_align_up((size_t)active * sizeof(int64_t), 16) + (size_t)active * sizeof(int4);
}

extern "C" int sr_mesh_count(const void* tsdf_values, int X, int Y, int Z, float level, void* count_scratch,
                             size_t count_scratch_bytes_, int64_t* totals, void* stream_) {
  Params P;
  if (!fill_params(P, tsdf_values, X, Y, Z, level) || !count_scratch || !totals) return SR_ERR_INVALID_ARGUMENT;
  if (count_scratch_bytes_ < count_scratch_bytes(P.nbricks) || ((uintptr_t)count_scratch & 15))
    return SR_ERR_WORKSPACE_TOO_SMALL;
  if (P.nbricks > 0x7fffffff) return SR_ERR_UNSUPPORTED;
  bind_count_scratch(P, count_scratch);
  P.totals = totals;
  hipStream_t s = (hipStream_t)stream_;
  if (vec_path(tsdf_values, Z))
    hipLaunchKernelGGL(sr_mesh_count_kernel<true>, dim3((unsigned)P.nbricks), dim3(kThreads), 0, s, P);
  else
    hipLaunchKernelGGL(sr_mesh_count_kernel<false>, dim3((unsigned)P.nbricks), dim3(kThreads), 0, s, P);
  hipLaunchKernelGGL(sr_mesh_scan_kernel, dim3(1), dim3(1024), 0, s, P);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_mesh_emit(const void* tsdf_values, int X, int Y, int Z, float level, float origin_x, float origin_y,
                            float origin_z, float scale, const void* count_scratch, size_t count_scratch_bytes_,
                            void* list_scratch, size_t list_scratch_bytes, int64_t active, int64_t num_vertices,
                            int64_t num_faces, float* vertices, float* normals, int* faces, void* stream_) {
  Params P;
  if (!fill_params(P, tsdf_values, X, Y, Z, level) || !count_scratch) return SR_ERR_INVALID_ARGUMENT;
  if (active < 0 || num_vertices < 0 || num_faces < 0) return SR_ERR_INVALID_ARGUMENT;
  if (num_vertices >= (int64_t)1 << 31 || num_faces >= (int64_t)1 << 31) return SR_ERR_UNSUPPORTED;
  if (active == 0) return SR_OK;
  if (!list_scratch || (num_vertices && !vertices) || (num_faces && !faces)) return SR_ERR_INVALID_ARGUMENT;
  if (count_scratch_bytes_ < count_scratch_bytes(P.nbricks) || list_scratch_bytes < sr_mesh_list_scratch_bytes(active) ||
      ((uintptr_t)count_scratch & 15) || ((uintptr_t)list_scratch & 15))
    return SR_ERR_WORKSPACE_TOO_SMALL;
  if (P.nbricks > 0x7fffffff || (active + kThreads - 1) / kThreads > 0x7fffffff) return SR_ERR_UNSUPPORTED;
  bind_count_scratch(P, const_cast<void*>(count_scratch));
  P.keys = (int64_t*)list_scratch;
  P.meta = (int4*)((char*)list_scratch + sr_align_up((size_t)active * sizeof(int64_t), 16));
  P.A = active; P.V = num_vertices; P.F = num_faces;
  P.ox = origin_x; P.oy = origin_y; P.oz = origin_z; P.scale = scale;
  P.verts = vertices; P.normals = num_vertices ? normals : nullptr; P.faces = faces;
  hipStream_t s = (hipStream_t)stream_;
  if (vec_path(tsdf_values, Z))
    hipLaunchKernelGGL(sr_mesh_compact_kernel<true>, dim3((unsigned)P.nbricks), dim3(kThreads), 0, s, P);
  else
    hipLaunchKernelGGL(sr_mesh_compact_kernel<false>, dim3((unsigned)P.nbricks), dim3(kThreads), 0, s, P);
  hipLaunchKernelGGL(sr_mesh_emit_kernel, dim3((unsigned)((active + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, P);
  return sr_hip_rc(hipGetLastError());
}
