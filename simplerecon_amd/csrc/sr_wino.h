// sr_wino.h -- definitions of the Winograd F(2x2, 3x3) kernel (sr_wino.hip: 4 waves, two workgroups per CU).
#pragma once
#include <stdio.h>
#include <stdlib.h>

#include "sr_common.h"
#include "sr_buffer.h"

#ifndef SR_WINO_WAVES
#define SR_WINO_WAVES 2  // waves per SIMD the register allocation must allow (2 = two workgroups per CU)
#endif

#ifndef SR_WINO_NT1_WAVES
#define SR_WINO_NT1_WAVES 2  // the same for the 32-output-channel instantiation (64 accumulator registers, 46 KB of LDS)
#endif

#ifndef SR_WINO_NB
#define SR_WINO_NB 4   // rotating weight-fragment register sets; must divide the 8 steps of a slab
#define SR_WINO_PD 3   // prefetch distance in steps (< NB)
#endif

#define WN_TR 4
#define WN_TC 8
#define WN_PH (2 * WN_TR + 2)  // 10 patch rows
#define WN_PW (2 * WN_TC + 2)  // 18 patch cols
#define WN_ROW 20              // floats per staged pixel / per V row (16 channels + 4 pad)
#define WN_RAW_FLOATS (WN_PH * WN_PW * WN_ROW)
#define WN_O_FLOATS(nt) (8 * 32 * 32 * (nt))
// Raw buffer A shares the first 64 KB with the epilogue slab O (A is dead by the epilogue); raw buffer B lives behind
// them so that the NEXT region's first slab can be staged while the current region finishes (its last MFMA phase and
// its epilogue): 78 KB, 2 workgroups per CU.
#define WN_V_FLOATS(nt) (WN_O_FLOATS(nt) - WN_RAW_FLOATS)   // offset of raw A: the tail of the O area
#define WN_LDS_FLOATS(nt) (WN_O_FLOATS(nt) + WN_RAW_FLOATS)
#define WN_STAGE_ELEMS (WN_PH * WN_PW * 4)  // float4 elements per slab (720)
#define WN_STAGE_PER_THREAD 3

struct SrWinoParams {
  const float* in; int64_t in_sb; int in_sp;
  const float* wu;                                  // packed U: [16][G][2][Co_pad][4]
  const float* bias;
  const float* res; int64_t res_sb; int res_sp;
  float* out; int64_t out_sb; int out_sp;
  int H, W, Cin, Cout, Co_pad, G;                   // stride 1, pad 1: output is H x W
  int regions_x, regions_y, co_blocks, total;
  float slope;
  int vec4;
  // split-K: a work item covers 1/ksplit of the input slabs and stores its raw partial output (no bias / residual /
  // activation) to part + ks * part_stride (dense channels-last [B, H*W, Cout]); sr_wino_reduce_kernel finishes.
  int ksplit; float* part; int64_t part_stride;
  int xcd_order;   // 1: items of a round are dealt to the XCDs in contiguous eighths (SR_WINO_XCD, default 1)
#ifdef SR_WINO_TRACE
  unsigned long long* trace;  // [blocks][SR_TR_REGIONS][SR_TR_EVENTS] shader-clock stamps (debug builds only)
#endif
};

// Launch note (sr_common.h) of an F(2x2) kernel with leading template arguments <nt, b[, c]>: p.total work items, each WN_TR x
// WN_TC tiles of 16 frequencies by 32 nt output channels over its K part's 16-channel slabs.
static inline SrLaunchNote sr_wino_note(int kernel, int nt, int b, int c, const SrWinoParams& p) {
  return {kernel, nt, b, c, 0, 0, 0, (int64_t)p.total * (WN_TR * WN_TC * 16), 32 * nt, (p.G / 2) * 16 / p.ksplit};
}

#ifdef SR_WINO_TRACE
#define SR_TR_REGIONS 12
#define SR_TR_EVENTS 16
#define SR_TR(ev)                                                                                          \
  do {                                                                                                     \
    if (tid == 0 && tr_region < SR_TR_REGIONS)                                                              \
      p.trace[((size_t)blockIdx.x * SR_TR_REGIONS + tr_region) * SR_TR_EVENTS + (ev)] = clock64();          \
  } while (0)
#else
#define SR_TR(ev) do {} while (0)
#endif

// float4 add / sub as two packed fp32 pairs (v_pk_add_f32): the transforms are pure add / sub work
typedef float wn_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float4 f4sub(float4 a, float4 b) {
  const wn_f2 lo = wn_f2{a.x, a.y} - wn_f2{b.x, b.y}, hi = wn_f2{a.z, a.w} - wn_f2{b.z, b.w};
  return make_float4(lo.x, lo.y, hi.x, hi.y);
}
__device__ __forceinline__ float4 f4add(float4 a, float4 b) {
  const wn_f2 lo = wn_f2{a.x, a.y} + wn_f2{b.x, b.y}, hi = wn_f2{a.z, a.w} + wn_f2{b.z, b.w};
  return make_float4(lo.x, lo.y, hi.x, hi.y);
}

// Buffer addressing, the 16-byte-store hazard and the 16-bit activation I/O: sr_buffer.h.  The F(2x2) kernels keep their
// staging and residual registers as HIP float4, so their loads go through this alias.
template <int IO>
__device__ __forceinline__ float4 wn_io_load(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  const sr_f4 v = sr_io_load<IO>(r, voff, soff);
  return make_float4(v.x, v.y, v.z, v.w);
}

// `SR_WN_PIN`: an empty asm that makes a value opaque at that point, so that addresses derived from it are formed there
// as register + immediate instead of being hoisted out of the loops, one register -- then one spill -- each.
#define SR_WN_PIN(...) asm volatile("" : __VA_ARGS__)

// ---- stages shared by sr_wino_kernel (sr_wino.hip) and its split-precision twin (sr_wino_split.hip) ----

// Region coordinates of work item wk of a grid of `xcd_g` workgroups, NT N-tiles per workgroup.
// XCD-aware work order.  Workgroup b runs on XCD b % 8 (round-robin dispatch) and each XCD has its own L2.  In round r
// the grid works on items [r G, (r + 1) G): give XCD x the CONTIGUOUS eighth [r G + x G/8, r G + (x + 1) G/8) of them
// (consecutive items are horizontally adjacent regions, G/8 of them about three region rows), so that the halo
// pixels two neighbouring regions share are fetched into ONE L2 instead of two (r02 PMC: 1.40x the algorithmic
// bytes).  The last, partial round keeps the plain order.
struct WnRegion { int b, oy0, ox0, co0, ks; };
template <int NT>
__device__ __forceinline__ WnRegion wn_decode(const SrWinoParams& p, int wk, int xcd_g) {
  if (p.xcd_order && (xcd_g & 7) == 0) {
    const int r0 = wk / xcd_g * xcd_g;
    if (r0 + xcd_g <= p.total) { const int bb = wk - r0; wk = r0 + (bb & 7) * (xcd_g >> 3) + (bb >> 3); }
  }
  WnRegion r;
  r.ks = wk % p.ksplit; wk /= p.ksplit;
  const int cb = wk % p.co_blocks; wk /= p.co_blocks;
  const int rx = wk % p.regions_x; wk /= p.regions_x;
  const int ry = wk % p.regions_y;
  r.b = wk / p.regions_y;
  r.oy0 = ry * (2 * WN_TR); r.ox0 = rx * (2 * WN_TC); r.co0 = cb * (32 * NT);
  return r;
}

// LDS side of the staging: element e -> pixel e >> 2, quad e & 3.  The 48 thread slots beyond the 720 elements of a
// patch write their (zero) registers into the pad quad of a pixel row instead of being branched around.
// st_lds0: slots 0 / 1 (+ it * 64 pixels), st_lds2: slot 2.
__device__ __forceinline__ void wn_stage_lds(int tid, int& st_lds0, int& st_lds2) {
  static_assert(WN_STAGE_PER_THREAD == 3 && 2 * 256 < WN_STAGE_ELEMS, "only the third slot of a thread can be a spare");
  st_lds0 = (tid >> 2) * WN_ROW + 4 * (tid & 3);
  st_lds2 = tid + 512 < WN_STAGE_ELEMS ? st_lds0 + 128 * WN_ROW : (tid + 512 - WN_STAGE_ELEMS) * WN_ROW + 16;
}
__device__ __forceinline__ void wn_stage_store(const float4 (&stg)[WN_STAGE_PER_THREAD], float* raw, int st_lds0, int st_lds2) {
  *reinterpret_cast<float4*>(&raw[st_lds0]) = stg[0];
  *reinterpret_cast<float4*>(&raw[st_lds0 + 64 * WN_ROW]) = stg[1];
  *reinterpret_cast<float4*>(&raw[st_lds2]) = stg[2];
}

// In-register input transform.  Wave w produces the frequency ROW ur = w of V = B^T d B (the rows it alone multiplies).
// Row ur of B^T d needs two patch rows: (0,2) d0-d2, (1,2) d1+d2, (2,1) d2-d1, (1,3) d1-d3.  Lane (i, kk) does it for
// tile i (the MFMA row it feeds) and the channel quads 2g + kk -- the A operands of its own MFMAs.
// The two patch rows are ONE register each (a, b): every other term of a load address is an immediate (left to itself
// the compiler hoists the 16 distinct addresses out of the work loop and spills them; see SR_WN_PIN).
__device__ __forceinline__ void wn_transform_role(int wave, int i, int kk, float& t_sign, int& rv_a, int& rv_b) {
  const int t_ra = wave == 0 ? 0 : (wave == 2 ? 2 : 1), t_rb = wave == 0 ? 2 : (wave == 1 ? 2 : (wave == 2 ? 1 : 3));
  t_sign = wave == 1 ? 1.0f : -1.0f;
  const int rv_base = ((2 * (i >> 3)) * WN_PW + 2 * (i & 7)) * WN_ROW + 4 * kk;   // patch offset of tile i, quad kk
  rv_a = rv_base + t_ra * WN_PW * WN_ROW;
  rv_b = rv_base + t_rb * WN_PW * WN_ROW;
}
__device__ __forceinline__ float4 wn_rv_fma(float t_sign, const float4 da, const float4 db) {
  const wn_f2 sg = {t_sign, t_sign};
  const wn_f2 lo = __builtin_elementwise_fma(sg, wn_f2{db.x, db.y}, wn_f2{da.x, da.y});
  const wn_f2 hi = __builtin_elementwise_fma(sg, wn_f2{db.z, db.w}, wn_f2{da.z, da.w});
  return make_float4(lo.x, lo.y, hi.x, hi.y);
}
__device__ __forceinline__ void wn_rv_ld(const float* raw, int rv_a, int rv_b, int g, int c, float4& da, float4& db) {
  da = *reinterpret_cast<const float4*>(&raw[rv_a + 8 * g + c * WN_ROW]);
  db = *reinterpret_cast<const float4*>(&raw[rv_b + 8 * g + c * WN_ROW]);
}
// wn_rv_row: the four frequencies uc = 0..3 of a row of B^T d from its four columns = the A operands of steps (g, uc).
__device__ __forceinline__ void wn_rv_row(const float4 (&w)[4], float4 (&a)[4]) {
  a[0] = f4sub(w[0], w[2]); a[1] = f4add(w[1], w[2]); a[2] = f4sub(w[2], w[1]); a[3] = f4sub(w[1], w[3]);
}

// ---- split-precision variant (sr_wino_split.hip; fenced experiment).  mode: 1 bf16, 2 f16 -- the split_format argument ----
int sr_wino_split_pack(const float* weight, int Cout, int Cin, float* packed, int mode, hipStream_t stream);
int sr_wino_split_launch(const SrWinoParams& p, int nt, int blocks, int mode, hipStream_t stream);
