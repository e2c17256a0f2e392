/* sr_view.h -- acceptance rules the convolution entry points apply to a channels-last view before they launch (host side,
 * plain C: tests/host/view_checks.c compiles it alone).  A view is (pointer, batch stride, pixel stride) with the strides
 * in ELEMENTS; a kernel that moves `quantum` channels per access needs every row to start on that boundary, and a kernel
 * that addresses an image through a buffer descriptor needs the image's byte span below 2^31.  DESIGN.md 3.3g. */
#pragma once
#include <stdint.h>

/* pointer aligned to mask + 1 bytes (mask = 15: float4, 7: four 16-bit channels) */
static inline int sr_ptr_aligned(const void* ptr, uintptr_t mask) { return ((uintptr_t)ptr & mask) == 0; }

/* every pixel row of every image starts aligned: the base pointer to mask + 1 bytes, both strides to `quantum` elements */
static inline int sr_rows_aligned(const void* ptr, int64_t batch_stride, int64_t pix_stride, uintptr_t mask, int quantum) {
  return sr_ptr_aligned(ptr, mask) && pix_stride % quantum == 0 && batch_stride % quantum == 0;
}

/* bytes from the first element of an image to the end of its last pixel's C channels, in 64-bit */
static inline int64_t sr_view_span(int64_t HW, int64_t pix_stride, int64_t C, int64_t elem_size) {
  return ((HW - 1) * pix_stride + C) * elem_size;
}

/* per-image byte offsets are 32-bit in buffer addressing (num_records and the lane offset) */
static inline int sr_span_fits32(int64_t span) { return span < ((int64_t)1 << 31); }

static inline int sr_view_fits32(int64_t HW, int64_t pix_stride, int64_t C, int64_t elem_size) {
  return sr_span_fits32(sr_view_span(HW, pix_stride, C, elem_size));
}
