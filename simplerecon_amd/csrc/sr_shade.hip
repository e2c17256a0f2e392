// sr_shade.hip -- colour and shaded renders of a triangle mesh from the rasteriser's face-id image, and the
// area-weighted vertex normals they need (gfx950).  Rules: include/simplerecon_hip.h, section "mesh shading";
// tests/shade_oracle.py restates both kernels in float64 numpy.
//
// The shading model is a stated one -- ambient plus Lambert over directional, point and head lights -- not pyrender's
// metallic-roughness shader: pyrender cannot be run next to this code, so nothing here claims to match its pictures.
//
// Deferred pass: one lane per pixel, 256 consecutive pixels of one view per workgroup, so the face-id reads and the
// planar fp32 writes coalesce; the three corners of the pixel's face are gathered (data-dependent, L2 for meshes that
// fit it).  The camera and the lights are the same for the whole workgroup: the lights arrive in the kernel arguments
// (the host has checked their kinds) and are moved to the camera frame once per workgroup, into LDS.  Everything per
// pixel is fp64 with contraction off, rounded to fp32 once.  The interleaved bytes are staged in LDS and leave as
// 32-bit words when the workgroup's first byte is word-aligned.
#include "sr_common.h"

namespace {

constexpr int kT = 256;

struct D3 {
  double x, y, z;
};

__device__ __forceinline__ D3 sub(const D3& a, const D3& b) {
#pragma clang fp contract(off)
  return {a.x - b.x, a.y - b.y, a.z - b.z};
}
__device__ __forceinline__ D3 cross(const D3& a, const D3& b) {
#pragma clang fp contract(off)
  return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}
__device__ __forceinline__ double dot(const D3& a, const D3& b) {
#pragma clang fp contract(off)
  return (a.x * b.x + a.y * b.y) + a.z * b.z;
}
__device__ __forceinline__ D3 scale(const D3& a, double s) {
#pragma clang fp contract(off)
  return {a.x * s, a.y * s, a.z * s};
}
__device__ __forceinline__ D3 over(const D3& a, double s) {
#pragma clang fp contract(off)
  return {a.x / s, a.y / s, a.z / s};
}
__device__ __forceinline__ D3 load3(const float* __restrict__ p) { return {(double)p[0], (double)p[1], (double)p[2]}; }
__device__ __forceinline__ bool finite(double v) { return v - v == 0.0; }
__device__ __forceinline__ bool finite3(const D3& a) { return finite(a.x) && finite(a.y) && finite(a.z); }

// x0 w0 + (x1 w1 + x2 w2): the value does not change when corners 1 and 2 trade places (a face with reversed winding)
__device__ __forceinline__ D3 blend(const float* __restrict__ attr, int64_t i0, int64_t i1, int64_t i2, double w0,
                                    double w1, double w2) {
#pragma clang fp contract(off)
  const D3 a = load3(attr + 3 * i0), b = load3(attr + 3 * i1), c = load3(attr + 3 * i2);
  return {a.x * w0 + (b.x * w1 + c.x * w2), a.y * w0 + (b.y * w1 + c.y * w2), a.z * w0 + (b.z * w1 + c.z * w2)};
}

struct Camera {
  double r[9], t[3];
};

__device__ __forceinline__ Camera load_camera(const float* __restrict__ T) {
  Camera c;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    c.r[3 * i + 0] = T[4 * i + 0];
    c.r[3 * i + 1] = T[4 * i + 1];
    c.r[3 * i + 2] = T[4 * i + 2];
    c.t[i] = T[4 * i + 3];
  }
  return c;
}

__device__ __forceinline__ D3 rotate(const Camera& c, const D3& p) {
#pragma clang fp contract(off)
  return {(c.r[0] * p.x + c.r[1] * p.y) + c.r[2] * p.z, (c.r[3] * p.x + c.r[4] * p.y) + c.r[5] * p.z,
          (c.r[6] * p.x + c.r[7] * p.y) + c.r[8] * p.z};
}
__device__ __forceinline__ D3 to_camera(const Camera& c, const D3& p) {
#pragma clang fp contract(off)
  const D3 q = rotate(c, p);
  return {q.x + c.t[0], q.y + c.t[1], q.z + c.t[2]};
}

struct ShadeArgs {
  const float* verts;
  const int32_t* faces;
  const float* K;
  const float* T;
  const int32_t* face;     // [B,H,W]
  const float* colors;     // [V,3] or null
  const float* normals;    // [V,3] or null
  float* out_f32;          // [B,3,H,W] or null
  uint8_t* out_u8;         // [B,H,W,3] or null
  float* normals_out;      // [B,3,H,W] or null
  int64_t V, F, HW, chunks;
  int W, num_lights, shading, flat;
  float off, ambient, base[3], bg[3];
  float lights[SR_SHADE_MAX_LIGHTS][SR_SHADE_LIGHT_FLOATS];
};

__device__ __forceinline__ float unit_clamp(double v) {   // [0, 1], NaN -> 0
  const float o = (float)v;
  return o >= 0.0f ? (o <= 1.0f ? o : 1.0f) : 0.0f;
}

// (uint8)(v * 255.0f), truncated (sr_viz's rule); the clamp only matters for a background outside [0, 1]
__device__ __forceinline__ uint8_t pixel8(float v) {
  const float s = __fmul_rn(v, 255.0f);
  return (uint8_t)(s >= 0.0f ? (s <= 255.0f ? (int)s : 255) : 0);
}

__global__ void __launch_bounds__(kT) sr_raster_shade_kernel(const ShadeArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_light[SR_SHADE_MAX_LIGHTS][3];   // camera frame: the unit vector towards a directional light,
                                                       // the position of a point light
  __shared__ uint32_t s_bytes[kT * 3 / 4];
  const int64_t block = blockIdx.x;
  const int b = (int)(block / a.chunks);
  const int64_t p0 = (block % a.chunks) * kT;
  const Camera cam = load_camera(a.T + (int64_t)b * 16);
  const float* k = a.K + (int64_t)b * 16;
  const double fx = k[0], fy = k[5], cxs = (double)k[2] - (double)a.off, cys = (double)k[6] - (double)a.off;

  if ((int)threadIdx.x < a.num_lights) {
    const float* L = a.lights[threadIdx.x];
    const int kind = (int)L[0];
    D3 v = load3(L + 1);
    if (kind == SR_SHADE_LIGHT_DIRECTIONAL) {
      const D3 d = rotate(cam, over(v, sqrt(dot(v, v))));
      v = {-d.x, -d.y, -d.z};
    } else if (kind == SR_SHADE_LIGHT_POINT) {
      v = to_camera(cam, v);
    }
    s_light[threadIdx.x][0] = v.x;
    s_light[threadIdx.x][1] = v.y;
    s_light[threadIdx.x][2] = v.z;
  }
  __syncthreads();

  const int64_t p = p0 + threadIdx.x;
  const bool active = p < a.HW;
  float out[3] = {a.bg[0], a.bg[1], a.bg[2]}, nout[3] = {0.0f, 0.0f, 0.0f};
  if (active) {
    const int64_t f = a.face[(int64_t)b * a.HW + p];
    int64_t i0 = -1, i1 = -1, i2 = -1;
    if (f >= 0 && f < a.F) {
      i0 = a.faces[3 * f];
      i1 = a.faces[3 * f + 1];
      i2 = a.faces[3 * f + 2];
    }
    if (i0 >= 0 && i0 < a.V && i1 >= 0 && i1 < a.V && i2 >= 0 && i2 < a.V) {
      // hit point and barycentrics from the ray (tests/raster_oracle.py, _cast_points)
      const D3 r = {((double)(p % a.W) - cxs) / fx, ((double)(p / a.W) - cys) / fy, 1.0};
      const D3 X0 = to_camera(cam, load3(a.verts + 3 * i0));
      const D3 e1 = sub(to_camera(cam, load3(a.verts + 3 * i1)), X0);
      const D3 e2 = sub(to_camera(cam, load3(a.verts + 3 * i2)), X0);
      const D3 n = cross(e1, e2);
      const double d = dot(r, n), an = dot(X0, n);
      const D3 P = scale(r, an / d);
      const double u = -dot(r, cross(X0, e2)) / d, v = -dot(r, cross(e1, X0)) / d;
      double w0 = fmin(fmax(1.0 - (u + v), 0.0), 1.0), w1 = fmin(fmax(u, 0.0), 1.0), w2 = fmin(fmax(v, 0.0), 1.0);
      const double ws = w0 + (w1 + w2);
      w0 /= ws;
      w1 /= ws;
      w2 /= ws;
      // normal: n . P has the sign of X0 . n, the rasteriser's plane constant c -- back-facing when c >= 0
      const bool back = an >= 0.0;
      D3 ng = over(n, sqrt(dot(n, n)));
      if (dot(ng, P) > 0.0) ng = {-ng.x, -ng.y, -ng.z};
      D3 nn = ng;
      if (a.normals && !a.flat) {
        const D3 m = rotate(cam, blend(a.normals, i0, i1, i2, w0, w1, w2));
        const double len = sqrt(dot(m, m));
        if (len >= 1e-12 && finite(len)) {
          nn = over(m, len);
          if (back) nn = {-nn.x, -nn.y, -nn.z};
        }
      }
      nout[0] = (float)nn.x;
      nout[1] = (float)nn.y;
      nout[2] = (float)nn.z;
      D3 c = {(double)a.base[0], (double)a.base[1], (double)a.base[2]};
      if (a.colors) c = blend(a.colors, i0, i1, i2, w0, w1, w2);
      if (a.shading == SR_SHADE_NORMALS) {
        c = {0.5 * (1.0 + nn.x), 0.5 * (1.0 + nn.y), 0.5 * (1.0 + nn.z)};
      } else if (a.shading == SR_SHADE_LAMBERT) {
        D3 sum = {0.0, 0.0, 0.0};
        for (int l = 0; l < a.num_lights; ++l) {
          const float* L = a.lights[l];
          const int kind = (int)L[0];
          D3 dir = {s_light[l][0], s_light[l][1], s_light[l][2]};
          double att = 1.0;
          if (kind == SR_SHADE_LIGHT_POINT) {
            const D3 to = sub(dir, P);
            const double d2 = dot(to, to);
            dir = over(to, sqrt(d2));
            att = 1.0 / fmax(d2, 1e-12);
          } else if (kind == SR_SHADE_LIGHT_HEAD) {
            const D3 h = over(P, sqrt(dot(P, P)));
            dir = {-h.x, -h.y, -h.z};
          }
          const double s = fmax(0.0, dot(nn, dir)) * att;   // (fmax: a NaN cosine lights nothing)
          sum.x = sum.x + (double)L[4] * s;
          sum.y = sum.y + (double)L[5] * s;
          sum.z = sum.z + (double)L[6] * s;
        }
        const double amb = a.ambient;
        c = {c.x * (amb + sum.x), c.y * (amb + sum.y), c.z * (amb + sum.z)};
      }
      out[0] = unit_clamp(c.x);
      out[1] = unit_clamp(c.y);
      out[2] = unit_clamp(c.z);
    }
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int64_t o = ((int64_t)b * 3 + ch) * a.HW + p;
      if (a.out_f32) a.out_f32[o] = out[ch];
      if (a.normals_out) a.normals_out[o] = nout[ch];
    }
  }
  if (a.out_u8) {   // (the same for the whole workgroup)
    uint8_t* s8 = (uint8_t*)s_bytes;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) s8[threadIdx.x * 3 + ch] = pixel8(out[ch]);
    __syncthreads();
    uint8_t* dst = a.out_u8 + ((int64_t)b * a.HW + p0) * 3;
    const int bytes = (int)min((int64_t)kT, a.HW - p0) * 3;
    const int words = ((uintptr_t)dst & 3) == 0 ? bytes / 4 : 0;
    if ((int)threadIdx.x < words) ((uint32_t*)dst)[threadIdx.x] = s_bytes[threadIdx.x];
    for (int i = words * 4 + threadIdx.x; i < bytes; i += kT) dst[i] = s8[i];
  }
}

// One thread per vertex: the sum of the cross products of its faces, in ascending face order.
__global__ void __launch_bounds__(kT) sr_mesh_vertex_normals_kernel(const float* __restrict__ verts, int64_t V,
                                                                    const int32_t* __restrict__ faces, int64_t F,
                                                                    const int64_t* __restrict__ order,
                                                                    const int64_t* __restrict__ offsets,
                                                                    float* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t v = (int64_t)blockIdx.x * kT + threadIdx.x;
  if (v >= V) return;
  int64_t k0 = offsets[v], k1 = offsets[v + 1];
  k0 = k0 < 0 ? 0 : k0;
  k1 = k1 > 3 * F ? 3 * F : k1;
  D3 s = {0.0, 0.0, 0.0};
  for (int64_t k = k0; k < k1; ++k) {
    const int64_t corner = order[k];
    if (corner < 0 || corner >= 3 * F) continue;
    const int64_t f = corner / 3;
    const int64_t i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
    if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) continue;
    if (faces[corner] != v) continue;   // (an order that does not belong to these faces)
    const D3 x0 = load3(verts + 3 * i0);
    const D3 n = cross(sub(load3(verts + 3 * i1), x0), sub(load3(verts + 3 * i2), x0));
    if (!finite3(n)) continue;
    s.x = s.x + n.x;
    s.y = s.y + n.y;
    s.z = s.z + n.z;
  }
  const double len = sqrt(dot(s, s));
  const bool ok = len > 0.0 && finite(len);
  out[3 * v + 0] = ok ? (float)(s.x / len) : 0.0f;
  out[3 * v + 1] = ok ? (float)(s.y / len) : 0.0f;
  out[3 * v + 2] = ok ? (float)(s.z / len) : 0.0f;
}

}  // namespace

extern "C" int sr_mesh_vertex_normals(const float* vertices, int64_t num_vertices, const int32_t* faces, int64_t num_faces,
                                      const int64_t* corner_order, const int64_t* vertex_offsets, float* normals,
                                      void* stream) {
  if (!vertices || !faces || !corner_order || !vertex_offsets || !normals) return SR_ERR_INVALID_ARGUMENT;
  if (num_vertices < 1 || num_vertices >= ((int64_t)1 << 31) || num_faces < 1 || num_faces >= ((int64_t)1 << 31))
    return SR_ERR_INVALID_ARGUMENT;
  const int64_t g = (num_vertices + kT - 1) / kT;
  hipLaunchKernelGGL(sr_mesh_vertex_normals_kernel, dim3((unsigned)g), dim3(kT), 0, (hipStream_t)stream, vertices,
                     num_vertices, faces, num_faces, corner_order, vertex_offsets, normals);
  return sr_hip_rc(hipGetLastError());
}

extern "C" int sr_raster_shade(const float* vertices, int64_t num_vertices, const int32_t* faces, int64_t num_faces,
                               const float* K, const float* cam_T_world, int B, int H, int W, float pixel_offset,
                               const int32_t* face_bhw, const float* colors, const float* normals,
                               const float* base_color, const float* background, float ambient, const float* lights,
                               int num_lights, int shading, int normal_mode, float* out_f32, uint8_t* out_u8,
                               float* normals_out, void* stream) {
  if (!vertices || !faces || !K || !cam_T_world || !face_bhw || !base_color || !background)
    return SR_ERR_INVALID_ARGUMENT;
  if (!out_f32 && !out_u8 && !normals_out) return SR_ERR_INVALID_ARGUMENT;
  if (num_vertices < 1 || num_vertices >= ((int64_t)1 << 31) || num_faces < 1 || num_faces >= ((int64_t)1 << 31))
    return SR_ERR_INVALID_ARGUMENT;
  if (B < 1 || H < 1 || W < 1 || H > SR_RASTER_MAX_SIDE || W > SR_RASTER_MAX_SIDE) return SR_ERR_INVALID_ARGUMENT;
  if (!(pixel_offset >= -1.0f && pixel_offset <= 1.0f)) return SR_ERR_INVALID_ARGUMENT;
  if (shading != SR_SHADE_UNLIT && shading != SR_SHADE_NORMALS && shading != SR_SHADE_LAMBERT)
    return SR_ERR_INVALID_ARGUMENT;
  if (normal_mode != SR_SHADE_NORMAL_SMOOTH && normal_mode != SR_SHADE_NORMAL_FLAT) return SR_ERR_INVALID_ARGUMENT;
  if (num_lights < 0 || num_lights > SR_SHADE_MAX_LIGHTS || (num_lights > 0 && !lights)) return SR_ERR_INVALID_ARGUMENT;
  ShadeArgs a;
  for (int l = 0; l < num_lights; ++l) {
    const float kind = lights[l * SR_SHADE_LIGHT_FLOATS];
    if (kind != (float)SR_SHADE_LIGHT_DIRECTIONAL && kind != (float)SR_SHADE_LIGHT_POINT &&
        kind != (float)SR_SHADE_LIGHT_HEAD)
      return SR_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < SR_SHADE_LIGHT_FLOATS; ++i) a.lights[l][i] = lights[l * SR_SHADE_LIGHT_FLOATS + i];
  }
  for (int l = num_lights; l < SR_SHADE_MAX_LIGHTS; ++l)
    for (int i = 0; i < SR_SHADE_LIGHT_FLOATS; ++i) a.lights[l][i] = 0.0f;
  const int64_t HW = (int64_t)H * W;
  const int64_t chunks = (HW + kT - 1) / kT;
  if ((int64_t)B * chunks * kT > SR_RASTER_MAX_THREADS) return SR_ERR_INVALID_ARGUMENT;
  a.verts = vertices;
  a.faces = faces;
  a.K = K;
  a.T = cam_T_world;
  a.face = face_bhw;
  a.colors = colors;
  a.normals = normals;
  a.out_f32 = out_f32;
  a.out_u8 = out_u8;
  a.normals_out = normals_out;
  a.V = num_vertices;
  a.F = num_faces;
  a.HW = HW;
  a.chunks = chunks;
  a.W = W;
  a.num_lights = num_lights;
  a.shading = shading;
  a.flat = normal_mode == SR_SHADE_NORMAL_FLAT;
  a.off = pixel_offset;
  a.ambient = ambient;
  for (int i = 0; i < 3; ++i) {
    a.base[i] = base_color[i];
    a.bg[i] = background[i];
  }
  hipLaunchKernelGGL(sr_raster_shade_kernel, dim3((unsigned)(B * chunks)), dim3(kT), 0, (hipStream_t)stream, a);
  return sr_hip_rc(hipGetLastError());
}
