// sr_mc.h -- the marching-cubes cube rules shared by the dense (sr_mesh.hip) and sparse (sr_sparse_tsdf.hip) mesh
// extraction: edge / face tables, the per-cube loop construction with the asymptotic decider, the fan triangulation with
// degenerate-triangle removal, and the per-voxel edge mask / triangle count.  The rules are stated in
// include/simplerecon_hip.h, section "mesh extraction".  Everything lives in an anonymous namespace: one copy per
// translation unit.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// edge parameters, positions and the asymptotic decider are separate fp32 operations, as in the numpy rules
#pragma clang fp contract(off)

namespace {

// Cube corners c = dx | dy << 1 | dz << 2.  The 12 edges are numbered by (owning corner in (dx, dy, dz) lexicographic
// order, axis): the same order as their global vertex indices.  Nibble e of kEdgeLo: the edge's lower corner.
constexpr uint64_t kEdgeLo = 0x351162244000ull;   // 0,0,0,4,4,2,2,6,1,1,5,3
constexpr uint32_t kEdgeAx = 0x992124u;           // 2 bits per edge: 0,1,2,0,1,0,2,0,1,2,1,2
// Faces: corners in counter-clockwise order seen from outside the cube, and the edge from corner k to corner k+1.
constexpr int kFaceC[6][4] = {{0, 4, 6, 2}, {1, 3, 7, 5}, {0, 1, 5, 4}, {2, 6, 7, 3}, {0, 2, 3, 1}, {4, 5, 7, 6}};
constexpr int kFaceE[6][4] = {{2, 4, 6, 1}, {8, 11, 10, 9}, {0, 9, 3, 2}, {6, 7, 11, 5}, {1, 5, 8, 0}, {3, 10, 7, 4}};

__device__ __forceinline__ int edge_lo(int e) { return (int)((kEdgeLo >> (4 * e)) & 15); }
__device__ __forceinline__ int edge_ax(int e) { return (int)((kEdgeAx >> (2 * e)) & 3); }

__device__ __forceinline__ float clamp1(float v) { return v < -1.0f ? -1.0f : (v > 1.0f ? 1.0f : v); }  // NaN stays
__device__ __forceinline__ bool crosses(float a, float b, float level) {
  return !isnan(a) && !isnan(b) && ((a < level) != (b < level));
}

// One cube: its crossing edges, their parameters t and the successor of every crossing edge on its loop.
struct Cube {
  uint32_t cross;  // bit e: edge e has a vertex
  uint64_t next;   // nibble e: the edge after e on its loop
  float t[12];
};

__device__ __forceinline__ void cube_build(const float c[8], float level, Cube& q) {
  q.cross = 0;
  q.next = 0;
  bool nan = false;
#pragma unroll
  for (int k = 0; k < 8; ++k) nan |= isnan(c[k]);
  if (nan) return;  // a cube with a non-finite corner emits nothing
#pragma unroll
  for (int e = 0; e < 12; ++e) {
    const float v0 = c[edge_lo(e)], v1 = c[edge_lo(e) | (1 << edge_ax(e))];
    q.t[e] = 0.0f;
    if ((v0 < level) != (v1 < level)) {
      q.cross |= 1u << e;
      q.t[e] = (level - v0) / (v1 - v0);
    }
  }
  if (!q.cross) return;
#pragma unroll
  for (int f = 0; f < 6; ++f) {
    bool up[4];
    int ncross = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) up[k] = !(c[kFaceC[f][k]] < level);
#pragma unroll
    for (int k = 0; k < 4; ++k) ncross += up[k] != up[(k + 1) & 3];
    // a segment runs from an edge where the counter-clockwise walk goes above -> below to one where it goes below ->
    // above: the surface then winds counter-clockwise seen from the above side
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (!(up[k] && !up[(k + 1) & 3])) continue;
      int end = 0;
      if (ncross == 2) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
          if (!up[m] && up[(m + 1) & 3]) end = kFaceE[f][m];
      } else {  // ambiguous face: above corners k, k+2; below corners k+1, k+3 (asymptotic decider)
        const float a = c[kFaceC[f][k]] - level, cc = c[kFaceC[f][(k + 2) & 3]] - level;
        const float b = c[kFaceC[f][(k + 1) & 3]] - level, d = c[kFaceC[f][(k + 3) & 3]] - level;
        end = (a * cc >= b * d) ? kFaceE[f][(k + 1) & 3] : kFaceE[f][(k + 3) & 3];
      }
      q.next |= (uint64_t)end << (4 * kFaceE[f][k]);
    }
  }
}

struct Pos { float x, y, z; };

__device__ __forceinline__ Pos edge_pos(const Cube& q, int e, int i, int j, int k) {
  const int lo = edge_lo(e), ax = edge_ax(e);
  Pos p{(float)(i + (lo & 1)), (float)(j + ((lo >> 1) & 1)), (float)(k + ((lo >> 2) & 1))};
  if (ax == 0) p.x = p.x + q.t[e];
  else if (ax == 1) p.y = p.y + q.t[e];
  else p.z = p.z + q.t[e];
  return p;
}

__device__ __forceinline__ bool same(const Pos& a, const Pos& b) { return a.x == b.x && a.y == b.y && a.z == b.z; }

// Walks the loops of the cube at voxel (i,j,k); each loop is a fan from its smallest edge (= smallest global vertex
// index).  emit(a, b, c) gets the edges of every non-degenerate triangle, in output order.
template <class Emit>
__device__ __forceinline__ int cube_triangles(const Cube& q, int i, int j, int k, Emit emit) {
  int ntri = 0;
  uint32_t seen = 0;
#pragma unroll 1
  for (int e0 = 0; e0 < 12; ++e0) {
    if (!((q.cross >> e0) & 1) || ((seen >> e0) & 1)) continue;
    const Pos p0 = edge_pos(q, e0, i, j, k);
    int b = (int)((q.next >> (4 * e0)) & 15);
    int c = (int)((q.next >> (4 * b)) & 15);
    seen |= (1u << e0) | (1u << b);
    Pos pb = edge_pos(q, b, i, j, k);
#pragma unroll 1
    for (int guard = 0; c != e0 && guard < 12; ++guard) {
      seen |= 1u << c;
      const Pos pc = edge_pos(q, c, i, j, k);
      if (!same(p0, pb) && !same(pb, pc) && !same(p0, pc)) {
        emit(e0, b, c);
        ++ntri;
      }
      b = c;
      pb = pc;
      c = (int)((q.next >> (4 * c)) & 15);
    }
  }
  return ntri;
}

struct NoEmit {
  __device__ void operator()(int, int, int) const {}
};

// Edge mask (bits x, y, z of the voxel's own edges) and triangle count of voxel (i,j,k) from its cube's corner values
// c[dx | dy << 1 | dz << 2]; hx / hy / hz: the neighbour along that axis exists.
__device__ __forceinline__ void voxel_info(const float c[8], bool hx, bool hy, bool hz, float level, int i, int j, int k,
                                           int& mask, int& ntri) {
  mask = (hx && crosses(c[0], c[1], level) ? 1 : 0) | (hy && crosses(c[0], c[2], level) ? 2 : 0) |
         (hz && crosses(c[0], c[4], level) ? 4 : 0);
  ntri = 0;
  if (!(hx && hy && hz)) return;
  bool any_below = false, any_above = false;
#pragma unroll
  for (int m = 0; m < 8; ++m) {
    any_below |= c[m] < level;
    any_above |= !(c[m] < level);
  }
  if (!(any_below && any_above)) return;
  Cube q;
  cube_build(c, level, q);
  if (q.cross) ntri = cube_triangles(q, i, j, k, NoEmit{});
}

}  // namespace
