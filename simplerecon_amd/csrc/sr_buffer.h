// sr_buffer.h -- buffer-descriptor addressing and 16-bit activation I/O shared by the matrix kernels (sr_wino*.hip,
// sr_pw*.hip, sr_dot_volume_lds.hip); device code, include after sr_common.h.  DESIGN.md 3.3g.
#pragma once
#include "sr_common.h"

typedef float sr_f4 __attribute__((ext_vector_type(4)));
typedef unsigned int sr_u4 __attribute__((ext_vector_type(4)));
typedef unsigned int sr_u2 __attribute__((ext_vector_type(2)));

// ---- buffer addressing (r04) ----------------------------------------------------------------------------------------
// Every VALU instruction a kernel issues outside its MFMA stream costs ~13 clocks while the co-resident workgroup
// keeps the matrix pipe busy, and r03's Winograd epilogue + prologue issued ~680 of them per region
// (64-bit address arithmetic, eight predicated residual-load / store branches, a 3 x division-by-18 re-aim of the staging
// loads).  The vector kernels address global memory through buffer descriptors: a wave-uniform descriptor (image base,
// byte range) + a 32-bit lane offset + a scalar offset operand.  A lane is switched off by its OFFSET (SR_OOB: the load
// returns 0, the store is dropped) instead of a branch, the per-(tile, pixel) deltas ride in the scalar offset operand
// (SALU work), and an interior region needs no per-lane predicate at all.  The byte range is 32-bit: the entry points
// refuse views whose per-image span does not fit (sr_view.h).
#define SR_RSRC_FLAGS 0x00020000      // raw buffer descriptor word 3 on gfx9-family parts
#define SR_OOB 0x7fffffffu            // a lane offset beyond any num_records
__device__ __forceinline__ __amdgpu_buffer_rsrc_t sr_rsrc(const void* base, int64_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)bytes, SR_RSRC_FLAGS);
}
__device__ __forceinline__ sr_f4 sr_buf_load(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  return __builtin_bit_cast(sr_f4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)voff, (int)soff, 0));
}
// Stores take their scalar delta through the LANE offset (`delta`: one v_add), not through the scalar-offset operand: a
// 16-byte buffer store reads its data registers some cycles after it issues, and a VALU write to them in that window
// corrupts the store ("VMEM store of more than 8 bytes" hazard, 2 wait states on gfx940+).  The compiler inserts those wait
// states only when the scalar-offset operand is NOT a register -- with an SGPR offset it assumes there is no hazard, and on
// gfx950 there is: the border-region epilogue of the F(2x2) Winograd kernel, which recomputes a lane offset between two
// stores, wrote the OFFSET into the first channel of the previous store (found by tests/test_gpu_image_encoder.py at
// 480x640, r04).
// (SR_OOB + delta stays below 2^32 and above every num_records: a switched-off lane stays switched off)
__device__ __forceinline__ void sr_buf_store(sr_f4 v, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned delta = 0u) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(sr_u4, v), r, (int)(voff + delta), 0, 0);
}

// ---- 16-bit activation I/O (r04; training under torch.autocast, reference options.py:100-101 / train.py:132) ----
// IO = 0: fp32 tensors (inference, the measured path).  IO = 1 / 2: the activation tensors are fp16 / bf16 in HBM -- four
// channels are ONE 8-byte load or store --, widened to fp32 on the way in and rounded (to nearest even) on the way out;
// weights, bias and the MFMA accumulation stay fp32.  Offsets are in bytes, so only the element size changes: SR_IO_ES(IO).
#define SR_IO_ES(io) ((io) == 0 ? 4u : 2u)
template <int IO>
__device__ __forceinline__ float sr_widen(unsigned short h) {
  if (IO == 1) return (float)__builtin_bit_cast(_Float16, h);
  return __builtin_bit_cast(float, (unsigned)h << 16);
}
template <int IO>
__device__ __forceinline__ unsigned short sr_narrow(float f) {
  if (IO == 1) return __builtin_bit_cast(unsigned short, (_Float16)f);
  return __builtin_bit_cast(unsigned short, (__bf16)f);
}
template <int IO>
__device__ __forceinline__ sr_f4 sr_io_load(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff) {
  if (IO == 0) return sr_buf_load(r, voff, soff);
  const sr_u2 v = __builtin_bit_cast(sr_u2, __builtin_amdgcn_raw_buffer_load_b64(r, (int)voff, (int)soff, 0));
  return sr_f4{sr_widen<IO>((unsigned short)(v.x & 0xffffu)), sr_widen<IO>((unsigned short)(v.x >> 16)),
               sr_widen<IO>((unsigned short)(v.y & 0xffffu)), sr_widen<IO>((unsigned short)(v.y >> 16))};
}
template <int IO>
__device__ __forceinline__ void sr_io_store(sr_f4 v, __amdgpu_buffer_rsrc_t r, unsigned voff, unsigned delta = 0u) {
  if (IO == 0) { sr_buf_store(v, r, voff, delta); return; }
  sr_u2 t;
  t.x = (unsigned)sr_narrow<IO>(v.x) | ((unsigned)sr_narrow<IO>(v.y) << 16);
  t.y = (unsigned)sr_narrow<IO>(v.z) | ((unsigned)sr_narrow<IO>(v.w) << 16);
  __builtin_amdgcn_raw_buffer_store_b64(t, r, (int)(voff + delta), 0, 0);
}
