// sr_sparse_tsdf.hip -- sparse colour TSDF fusion on 16^3-voxel blocks (the reference's Open3DFuser, tools/fusers_helper.py,
// on Open3D's ScalableTSDFVolume) and marching cubes across block borders with vertex colour.  gfx950 only.
//
// The rules are stated in include/simplerecon_hip.h, section "sparse TSDF"; tests/sparse_tsdf_oracle.py restates them in
// numpy.  The caller (simplerecon_amd/scalable_tsdf.py) keeps the sorted block table and the voxel pool; per call:
//   touch     : a thread per 4x4-subsampled pixel writes the keys of the up to 8 blocks its point touches.
//   masks     : after the caller's torch.unique, each workgroup collects the distinct blocks of 256 pixels of one
//               frame in LDS and ORs the frame bit into each block's uint64 once.
//   integrate : a workgroup per touched block, a thread per z-column of 16 voxels; the column's tsdf, weight and rgb are
//               read once into registers, every frame of the block's mask is applied there in order, and written once.
// Extraction: a workgroup per block stages the 17^3 values of the block and its +x/+y/+z neighbours (NaN where the
// weight is 0 or the block is missing) in LDS; one pass counts vertices and faces per block, a second writes vertices,
// colours and the vertex table, a third the faces (a face's vertices may belong to a neighbour block).
#include "sr_common.h"
#include "sr_block.h"
#include "sr_mc.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;          // a block's 16 x 16 z-columns
constexpr int kVox = 4096;             // voxels per block
constexpr int kHalo = 17;              // staged edge length: the block and one layer of its +x/+y/+z neighbours
constexpr int kHaloN = kHalo * kHalo * kHalo;
constexpr int64_t kKeyOff = 1ll << 20;
constexpr int64_t kKeyMask = (1ll << 21) - 1;

__device__ __forceinline__ int64_t pack_key(int64_t bx, int64_t by, int64_t bz) {
  return ((bx + kKeyOff) << 42) | ((by + kKeyOff) << 21) | (bz + kKeyOff);
}
__device__ __forceinline__ bool key_in_range(int64_t b) { return b >= -kKeyOff && b < kKeyOff; }
__device__ __forceinline__ void unpack_key(int64_t key, int& bx, int& by, int& bz) {
  bx = (int)(((key >> 42) & kKeyMask) - kKeyOff);
  by = (int)(((key >> 21) & kKeyMask) - kKeyOff);
  bz = (int)((key & kKeyMask) - kKeyOff);
}

// ---------------------------------------------------------------------------------------------------- touch (fp64)
__global__ __launch_bounds__(kThreads) void sr_stsdf_touch_kernel(const float* __restrict__ depth, int h, int w, int sw,
                                                                  int S, const double* __restrict__ frames_inv,
                                                                  double trunc, double unit, int64_t* cand) {
  const int s = blockIdx.x * kThreads + threadIdx.x;
  const int f = blockIdx.y;
  if (s >= S) return;
  int64_t* out = cand + ((int64_t)f * S + s) * 8;
  const int u = (s % sw) * 4, v = (s / sw) * 4;
  const double d = (double)depth[((int64_t)f * h + v) * w + u];
  int64_t lo[3], hi[3];
  bool ok = d > 0.0;
  if (ok) {
    const double* M = frames_inv + f * SR_STSDF_FRAME_FLOATS;
    const double fx = M[12], fy = M[13], cx = M[14], cy = M[15];
    const double x = (((double)u - cx) * d) / fx, y = (((double)v - cy) * d) / fy, z = d;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double p = ((M[4 * a] * x + M[4 * a + 1] * y) + M[4 * a + 2] * z) + M[4 * a + 3];
      const double l = floor((p - trunc) / unit), hh = floor((p + trunc) / unit);
      ok &= isfinite(l) && isfinite(hh) && fabs(l) < 0x1p40 && fabs(hh) < 0x1p40;  // safe to convert; range below
      lo[a] = ok ? (int64_t)l : 0;
      hi[a] = ok ? (int64_t)hh : 0;
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    int64_t key = SR_STSDF_KEY_NONE;
    if (ok) {
      const bool dup = ((k & 1) && hi[0] == lo[0]) || ((k & 2) && hi[1] == lo[1]) || ((k & 4) && hi[2] == lo[2]);
      const int64_t bx = (k & 1) ? hi[0] : lo[0], by = (k & 2) ? hi[1] : lo[1], bz = (k & 4) ? hi[2] : lo[2];
      if (!dup && key_in_range(bx) && key_in_range(by) && key_in_range(bz)) key = pack_key(bx, by, bz);
    }
    out[k] = key;
  }
}

// A workgroup covers 256 subsampled pixels of one frame (2048 candidates): their distinct blocks are collected in an
// LDS set first, so each block gets one global atomic OR per workgroup instead of one per candidate (a frame's pixels
// touch few blocks, and same-address atomics serialise).  The set has a slot per candidate: probing always ends.
constexpr int kMaskSet = 8 * kThreads;

__global__ __launch_bounds__(kThreads) void sr_stsdf_masks_kernel(const int64_t* __restrict__ cand,
                                                                  const int64_t* __restrict__ inverse, int S,
                                                                  unsigned long long* masks) {
  __shared__ unsigned long long set[kMaskSet];
  const int f = blockIdx.y;
  for (int i = threadIdx.x; i < kMaskSet; i += kThreads) set[i] = ~0ull;
  __syncthreads();
  const int s = blockIdx.x * kThreads + threadIdx.x;
  if (s < S) {
    const int64_t base = ((int64_t)f * S + s) * 8;
#pragma unroll 1
    for (int k = 0; k < 8; ++k) {
      if (cand[base + k] == SR_STSDF_KEY_NONE) continue;
      const unsigned long long u = (unsigned long long)inverse[base + k];
      unsigned h = (unsigned)(u * 0x9E3779B97F4A7C15ull >> 52) & (kMaskSet - 1);
      for (;;) {
        const unsigned long long prev = atomicCAS(&set[h], ~0ull, u);
        if (prev == ~0ull || prev == u) break;
        h = (h + 1) & (kMaskSet - 1);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kMaskSet; i += kThreads)
    if (set[i] != ~0ull) atomicOr(masks + set[i], 1ull << f);
}

// ---------------------------------------------------------------------------------------------- integrate (fp32)
struct IntegrateParams {
  float* pool;
  const int64_t* keys;
  const int64_t* slots;
  const unsigned long long* masks;
  const float* frames;
  const float* depth;
  const uint8_t* color;
  int B, h, w;
  float vl, trunc;
};

__global__ __launch_bounds__(kThreads) void sr_stsdf_integrate_kernel(IntegrateParams p) {
  __shared__ float sf[SR_STSDF_MAX_FRAMES * SR_STSDF_FRAME_FLOATS];
  for (int i = threadIdx.x; i < p.B * SR_STSDF_FRAME_FLOATS; i += kThreads) sf[i] = p.frames[i];
  __syncthreads();
  const int64_t slot = p.slots[blockIdx.x];
  if (slot < 0) return;  // the empty-candidate entry of the caller's unique keys: uniform over the workgroup
  const unsigned long long mask = p.masks[blockIdx.x];
  int bx, by, bz;
  unpack_key(p.keys[blockIdx.x], bx, by, bz);
  const int t = threadIdx.x, lx = t >> 4, ly = t & 15;
  float* col = p.pool + slot * (5 * kVox) + t * 16;
  float ts[16], wt[16], cr[16], cg[16], cb[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const float4 a = reinterpret_cast<const float4*>(col)[q];
    const float4 b = reinterpret_cast<const float4*>(col + kVox)[q];
    const float4 r = reinterpret_cast<const float4*>(col + 2 * kVox)[q];
    const float4 g = reinterpret_cast<const float4*>(col + 3 * kVox)[q];
    const float4 bl = reinterpret_cast<const float4*>(col + 4 * kVox)[q];
    ts[4 * q] = a.x; ts[4 * q + 1] = a.y; ts[4 * q + 2] = a.z; ts[4 * q + 3] = a.w;
    wt[4 * q] = b.x; wt[4 * q + 1] = b.y; wt[4 * q + 2] = b.z; wt[4 * q + 3] = b.w;
    cr[4 * q] = r.x; cr[4 * q + 1] = r.y; cr[4 * q + 2] = r.z; cr[4 * q + 3] = r.w;
    cg[4 * q] = g.x; cg[4 * q + 1] = g.y; cg[4 * q + 2] = g.z; cg[4 * q + 3] = g.w;
    cb[4 * q] = bl.x; cb[4 * q + 1] = bl.y; cb[4 * q + 2] = bl.z; cb[4 * q + 3] = bl.w;
  }
  const float x = ((float)(16 * bx + lx) + 0.5f) * p.vl;
  const float y = ((float)(16 * by + ly) + 0.5f) * p.vl;
  const float wlim = (float)p.w - 0.0001f, hlim = (float)p.h - 0.0001f;
  const int64_t plane = (int64_t)p.h * p.w;
#pragma unroll 1
  for (int f = 0; f < p.B; ++f) {
    if (!((mask >> f) & 1)) continue;  // uniform over the workgroup
    const float* F = sf + f * SR_STSDF_FRAME_FLOATS;
    const float fx = F[12], fy = F[13], cx = F[14], cy = F[15];
    // the x and y terms of each row are the same for the whole column: ((r0 x + r1 y) + r2 z) + t
    const float px0 = F[0] * x + F[1] * y, py0 = F[3] * x + F[4] * y, pz0 = F[6] * x + F[7] * y;
    const float* D = p.depth + f * plane;
    const uint8_t* C = p.color ? p.color + (int64_t)f * 3 * plane : nullptr;
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      const float z = ((float)(16 * bz + m) + 0.5f) * p.vl;
      const float px = (px0 + F[2] * z) + F[9], py = (py0 + F[5] * z) + F[10], pz = (pz0 + F[8] * z) + F[11];
      if (pz <= 0.0f) continue;
      const float uf = ((px * fx) / pz + cx) + 0.5f, vf = ((py * fy) / pz + cy) + 0.5f;
      if (!(uf >= 0.0001f && uf < wlim && vf >= 0.0001f && vf < hlim)) continue;
      const int u = (int)uf, v = (int)vf;
      const int64_t pix = (int64_t)v * p.w + u;
      const float d = D[pix];
      if (d <= 0.0f) continue;
      const float a = ((float)u - cx) / fx, b = ((float)v - cy) / fy;
      const float sdf = (d - pz) * sqrtf((1.0f + a * a) + b * b);
      if (!(sdf > -p.trunc)) continue;
      float tn = sdf / p.trunc;
      tn = tn < 1.0f ? tn : 1.0f;
      const float W = wt[m], W1 = W + 1.0f;
      const float r = C ? (float)C[pix] : 178.0f, g = C ? (float)C[plane + pix] : 178.0f,
                  bl = C ? (float)C[2 * plane + pix] : 178.0f;
      ts[m] = (ts[m] * W + tn) / W1;
      cr[m] = (cr[m] * W + r) / W1;
      cg[m] = (cg[m] * W + g) / W1;
      cb[m] = (cb[m] * W + bl) / W1;
      wt[m] = W1;
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    reinterpret_cast<float4*>(col)[q] = make_float4(ts[4 * q], ts[4 * q + 1], ts[4 * q + 2], ts[4 * q + 3]);
    reinterpret_cast<float4*>(col + kVox)[q] = make_float4(wt[4 * q], wt[4 * q + 1], wt[4 * q + 2], wt[4 * q + 3]);
    reinterpret_cast<float4*>(col + 2 * kVox)[q] = make_float4(cr[4 * q], cr[4 * q + 1], cr[4 * q + 2], cr[4 * q + 3]);
    reinterpret_cast<float4*>(col + 3 * kVox)[q] = make_float4(cg[4 * q], cg[4 * q + 1], cg[4 * q + 2], cg[4 * q + 3]);
    reinterpret_cast<float4*>(col + 4 * kVox)[q] = make_float4(cb[4 * q], cb[4 * q + 1], cb[4 * q + 2], cb[4 * q + 3]);
  }
}

// ------------------------------------------------------------------------------------------------------ extraction
enum MeshPass { kCount = 0, kVertices = 1, kFaces = 2 };

struct MeshParams {
  const float* pool;
  const int64_t* keys;
  const int64_t* slots;
  int64_t n;
  float vl;
  int32_t* counts;         // [2][n]
  const int64_t* offsets;  // [2][n]
  int64_t V, F;
  int32_t* vtab;           // [n][3][4096]
  float* verts;
  float* colors;
  int32_t* faces;
};

__device__ __forceinline__ float halo(const float* hv, int x, int y, int z) { return hv[(x * kHalo + y) * kHalo + z]; }

template <int PASS>
__global__ __launch_bounds__(kThreads) void sr_stsdf_mesh_kernel(MeshParams p) {
  __shared__ float hv[kHaloN];
  __shared__ int64_t nb_idx[8], nb_slot[8];  // neighbour c = dx | dy << 1 | dz << 2: sorted index and pool slot, or -1
  const int64_t n = blockIdx.x;
  int bx, by, bz;
  unpack_key(p.keys[n], bx, by, bz);
  const int t = threadIdx.x;
  if (t < 8) {
    const int dx = t & 1, dy = (t >> 1) & 1, dz = (t >> 2) & 1;
    int64_t idx = -1;
    if (t == 0) idx = n;
    else if (key_in_range(bx + dx) && key_in_range(by + dy) && key_in_range(bz + dz))
      idx = sr_find_sorted(p.keys, 0, p.n, pack_key(bx + dx, by + dy, bz + dz));
    nb_idx[t] = idx;
    nb_slot[t] = idx < 0 ? -1 : p.slots[idx];
  }
  __syncthreads();
  for (int i = t; i < kHaloN; i += kThreads) {
    const int x = i / (kHalo * kHalo), y = (i / kHalo) % kHalo, z = i % kHalo;
    const int c = (x >> 4) | ((y >> 4) << 1) | ((z >> 4) << 2);
    const int64_t slot = nb_slot[c];
    float v = __builtin_nanf("");
    if (slot >= 0) {
      const int l = (((x & 15) << 4) | (y & 15)) << 4 | (z & 15);
      const float* b = p.pool + slot * (5 * kVox);
      if (b[kVox + l] != 0.0f) v = clamp1(b[l]);
    }
    hv[i] = v;
  }
  __syncthreads();

  const int lx = t >> 4, ly = t & 15;
  const int gx = 16 * bx + lx, gy = 16 * by + ly;
  uint32_t info[4] = {0, 0, 0, 0};  // 8 bits per voxel: edge mask | triangles << 3
  int nv = 0, nt = 0;
#pragma unroll 1
  for (int m = 0; m < 16; ++m) {
    float c[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = halo(hv, lx + (k & 1), ly + ((k >> 1) & 1), m + ((k >> 2) & 1));
    int mask, ntri;
    voxel_info(c, true, true, true, 0.0f, gx, gy, 16 * bz + m, mask, ntri);
    info[m >> 2] |= (uint32_t)(mask | (ntri << 3)) << (8 * (m & 3));
    nv += __popc(mask);
    nt += ntri;
  }
  const int cnt[2] = {nv, nt};
  int excl[2], total[2];
  sr_block_scan<2, kThreads>(cnt, excl, total);
  if (PASS == kCount) {
    if (t == 0) {
      p.counts[n] = total[0];
      p.counts[p.n + n] = total[1];
    }
    return;
  }
  if (PASS == kVertices) {
    int64_t vi = p.offsets[n] + excl[0];
#pragma unroll 1
    for (int m = 0; m < 16; ++m) {
      const int mask = (int)(info[m >> 2] >> (8 * (m & 3))) & 7;
      const int l = (t << 4) | m;
#pragma unroll 1
      for (int a = 0; a < 3; ++a) {
        if (!((mask >> a) & 1)) continue;
        const int dx = a == 0, dy = a == 1, dz = a == 2;
        const float v0 = halo(hv, lx, ly, m), v1 = halo(hv, lx + dx, ly + dy, m + dz);
        const float tt = (0.0f - v0) / (v1 - v0);
        float q[3] = {(float)gx, (float)gy, (float)(16 * bz + m)};
        q[a] = q[a] + tt;
        // colours of both endpoints; the upper one may lie in the neighbour block along a
        const float* b0 = p.pool + nb_slot[0] * (5 * kVox);
        const int ux = lx + dx, uy = ly + dy, uz = m + dz;
        const int cu = (ux >> 4) | ((uy >> 4) << 1) | ((uz >> 4) << 2);
        const float* b1 = p.pool + (nb_slot[cu] >= 0 ? nb_slot[cu] : nb_slot[0]) * (5 * kVox);  // v1 finite: it exists
        const int l1 = (((ux & 15) << 4) | (uy & 15)) << 4 | (uz & 15);
        if (vi < p.V) {
#pragma unroll
          for (int d = 0; d < 3; ++d) {
            p.verts[3 * vi + d] = (q[d] + 0.5f) * p.vl;
            const float c0 = b0[(2 + d) * kVox + l], c1 = b1[(2 + d) * kVox + l1];
            p.colors[3 * vi + d] = (c0 + tt * (c1 - c0)) / 255.0f;
          }
        }
        p.vtab[(n * 3 + a) * kVox + l] = (int32_t)vi;
        ++vi;
      }
    }
    return;
  }
  // PASS == kFaces: every vertex table of this block and its neighbours was written by the previous launch
  int64_t fi = p.offsets[p.n + n] + excl[1];
#pragma unroll 1
  for (int m = 0; m < 16; ++m) {
    const int ntri = (int)(info[m >> 2] >> (8 * (m & 3) + 3)) & 31;
    if (!ntri) continue;
    float c[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) c[k] = halo(hv, lx + (k & 1), ly + ((k >> 1) & 1), m + ((k >> 2) & 1));
    Cube q;
    cube_build(c, 0.0f, q);
    int gid[12];
#pragma unroll
    for (int e = 0; e < 12; ++e) {
      gid[e] = -1;
      if (!((q.cross >> e) & 1)) continue;
      const int oc = edge_lo(e);
      const int ox = lx + (oc & 1), oy = ly + ((oc >> 1) & 1), oz = m + ((oc >> 2) & 1);
      const int cn = (ox >> 4) | ((oy >> 4) << 1) | ((oz >> 4) << 2);
      const int lo = (((ox & 15) << 4) | (oy & 15)) << 4 | (oz & 15);
      if (nb_idx[cn] >= 0) gid[e] = p.vtab[(nb_idx[cn] * 3 + edge_ax(e)) * kVox + lo];  // always: its corners are finite
    }
    cube_triangles(q, gx, gy, 16 * bz + m, [&](int a, int b, int cc) {
      if (fi < p.F) {
        p.faces[3 * fi + 0] = gid[a];
        p.faces[3 * fi + 1] = gid[b];
        p.faces[3 * fi + 2] = gid[cc];
      }
      ++fi;
    });
  }
}

bool aligned16(const void* ptr) { return ((uintptr_t)ptr & 15) == 0; }

}  // namespace

extern "C" int sr_stsdf_touch(const float* depth, int B, int h, int w, const double* frames_inv, double sdf_trunc,
                              double unit, int64_t* cand_keys, void* stream) {
  if (!depth || !frames_inv || !cand_keys || B < 1 || B > SR_STSDF_MAX_FRAMES || h < 1 || w < 1 || h > (1 << 15) ||
      w > (1 << 15))
    return SR_ERR_INVALID_ARGUMENT;
  if (!(sdf_trunc > 0.0) || !(unit > 2.0 * sdf_trunc)) return SR_ERR_INVALID_ARGUMENT;
  const int sw = (w + 3) / 4, S = sw * ((h + 3) / 4);
  hipLaunchKernelGGL(sr_stsdf_touch_kernel, dim3((S + kThreads - 1) / kThreads, B), dim3(kThreads), 0,
                     (hipStream_t)stream, depth, h, w, sw, S, frames_inv, sdf_trunc, unit, cand_keys);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_stsdf_block_masks(const int64_t* cand_keys, const int64_t* inverse, int64_t n_cand,
                                    int64_t cand_per_frame, uint64_t* masks, void* stream) {
  if (n_cand < 0 || cand_per_frame < 1 || (n_cand && (!cand_keys || !inverse || !masks)) ||
      n_cand > cand_per_frame * SR_STSDF_MAX_FRAMES || cand_per_frame % 8)
    return SR_ERR_INVALID_ARGUMENT;
  if (n_cand == 0) return SR_OK;
  if (n_cand % cand_per_frame || cand_per_frame / 8 > 0x7fffffff) return SR_ERR_INVALID_ARGUMENT;
  const int S = (int)(cand_per_frame / 8), B = (int)(n_cand / cand_per_frame);
  hipLaunchKernelGGL(sr_stsdf_masks_kernel, dim3((S + kThreads - 1) / kThreads, B), dim3(kThreads), 0,
                     (hipStream_t)stream, cand_keys, inverse, S, (unsigned long long*)masks);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_stsdf_integrate(float* pool, int64_t capacity, const int64_t* block_keys, const int64_t* block_slots,
                                  const uint64_t* block_masks, int64_t n_blocks, const float* frames, const float* depth,
                                  const uint8_t* color, int B, int h, int w, float voxel_length, float sdf_trunc,
                                  void* stream) {
  if (n_blocks < 0 || capacity < 0 || B < 1 || B > SR_STSDF_MAX_FRAMES || h < 1 || w < 1 || h > (1 << 15) ||
      w > (1 << 15) || !(voxel_length > 0.0f) || !(sdf_trunc > 0.0f))
    return SR_ERR_INVALID_ARGUMENT;
  if (n_blocks == 0) return SR_OK;
  if (!pool || !block_keys || !block_slots || !block_masks || !frames || !depth || !aligned16(pool))
    return SR_ERR_INVALID_ARGUMENT;
  if (n_blocks > 0x7fffffff) return SR_ERR_UNSUPPORTED;
  IntegrateParams P{pool, block_keys, block_slots, (const unsigned long long*)block_masks, frames, depth, color, B, h, w,
                    voxel_length, sdf_trunc};
  hipLaunchKernelGGL(sr_stsdf_integrate_kernel, dim3((unsigned)n_blocks), dim3(kThreads), 0, (hipStream_t)stream, P);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_stsdf_mesh_count(const float* pool, int64_t capacity, const int64_t* keys, const int64_t* slots,
                                   int64_t n_blocks, int32_t* block_counts, void* stream) {
  if (n_blocks < 0 || n_blocks > capacity) return SR_ERR_INVALID_ARGUMENT;
  if (n_blocks == 0) return SR_OK;
  if (!pool || !keys || !slots || !block_counts) return SR_ERR_INVALID_ARGUMENT;
  if (n_blocks > 0x7fffffff) return SR_ERR_UNSUPPORTED;
  MeshParams P{};
  P.pool = pool; P.keys = keys; P.slots = slots; P.n = n_blocks; P.counts = block_counts;
  hipLaunchKernelGGL(sr_stsdf_mesh_kernel<kCount>, dim3((unsigned)n_blocks), dim3(kThreads), 0, (hipStream_t)stream, P);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_stsdf_mesh_emit(const float* pool, int64_t capacity, const int64_t* keys, const int64_t* slots,
                                  int64_t n_blocks, float voxel_length, const int64_t* block_offsets,
                                  int64_t num_vertices, int64_t num_faces, int32_t* vertex_table, float* vertices,
                                  float* colors, int32_t* faces, void* stream) {
  if (n_blocks < 0 || n_blocks > capacity || num_vertices < 0 || num_faces < 0 || !(voxel_length > 0.0f))
    return SR_ERR_INVALID_ARGUMENT;
  if (num_vertices >= (int64_t)1 << 31 || num_faces >= (int64_t)1 << 31) return SR_ERR_UNSUPPORTED;
  if (n_blocks == 0 || num_vertices == 0) return SR_OK;
  if (!pool || !keys || !slots || !block_offsets || !vertex_table || !vertices || !colors || (num_faces && !faces))
    return SR_ERR_INVALID_ARGUMENT;
  if (n_blocks > 0x7fffffff) return SR_ERR_UNSUPPORTED;
  MeshParams P{};
  P.pool = pool; P.keys = keys; P.slots = slots; P.n = n_blocks; P.vl = voxel_length; P.offsets = block_offsets;
  P.V = num_vertices; P.F = num_faces; P.vtab = vertex_table; P.verts = vertices; P.colors = colors; P.faces = faces;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sr_stsdf_mesh_kernel<kVertices>, dim3((unsigned)n_blocks), dim3(kThreads), 0, s, P);
  if (num_faces)
    hipLaunchKernelGGL(sr_stsdf_mesh_kernel<kFaces>, dim3((unsigned)n_blocks), dim3(kThreads), 0, s, P);
  return sr_hip_rc(hipGetLastError());
}
