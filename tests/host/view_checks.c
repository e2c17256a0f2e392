/* Boundary checks of the acceptance predicates in csrc/sr_view.h, compiled with a plain C compiler and run by
 * tests/test_view_checks_host.py.  Exit status 0 and "view checks ok" when every check holds. */
#include <stdio.h>

#include "sr_view.h"

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      printf("FAILED line %d: %s\n", __LINE__, #cond);                \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

int main(void) {
  const int64_t lim = (int64_t)1 << 31;

  /* the span itself: ((HW - 1) * stride + C) * elem_size */
  CHECK(sr_view_span(1, 100, 16, 4) == 64);
  CHECK(sr_view_span(64, 16, 16, 4) == 64 * 64);
  CHECK(sr_view_span(64, 24, 16, 2) == (63 * 24 + 16) * 2);

  /* 4-byte elements, both sides of 2^31: 2^24 pixels at stride 32 */
  CHECK(sr_view_span(1 << 24, 32, 32, 4) == lim);
  CHECK(!sr_view_fits32(1 << 24, 32, 32, 4));
  CHECK(sr_view_span(1 << 24, 32, 28, 4) == lim - 16);
  CHECK(sr_view_fits32(1 << 24, 32, 28, 4));
  CHECK(sr_span_fits32(lim - 1) && !sr_span_fits32(lim) && !sr_span_fits32(lim + 1));

  /* 2-byte elements: the same view holds twice the pixels */
  CHECK(sr_view_fits32(1 << 24, 32, 32, 2));
  CHECK(sr_view_span(1 << 25, 32, 32, 2) == lim);
  CHECK(!sr_view_fits32(1 << 25, 32, 32, 2));
  CHECK(sr_view_fits32(1 << 25, 32, 24, 2));

  /* sizes whose product wraps in 32 bits and then looks small: a 16384 x 16384 map of 8 channels is 2^33 bytes
   * (0 modulo 2^32), and 65536 x 32768 pixels at stride 4 make 2^35 */
  CHECK(sr_view_span((int64_t)16384 * 16384, 8, 8, 4) == (int64_t)1 << 33);
  CHECK(!sr_view_fits32((int64_t)16384 * 16384, 8, 8, 4));
  CHECK(!sr_view_fits32((int64_t)16384 * 16384, 8, 8, 2));
  CHECK(!sr_view_fits32((int64_t)65536 * 32768, 4, 4, 4));
  CHECK(!sr_view_fits32(((int64_t)1 << 30) + 1, 4, 4, 4));   /* (2^30 + 1) * 16: 16 modulo 2^32 */

  /* the LDS-staged dot sweep: source maps of 64-byte texels (16 fp32 channels, dense); h * w = 2^25 is refused */
  CHECK(!sr_view_fits32((int64_t)1 << 25, 16, 16, 4));
  CHECK(sr_view_fits32(((int64_t)1 << 25) - 1, 16, 16, 4));
  CHECK(sr_view_span(((int64_t)1 << 25) - 1, 16, 16, 4) == lim - 64);
  CHECK(!sr_view_fits32((int64_t)8192 * 4096, 16, 16, 4) && sr_view_fits32((int64_t)8191 * 4096, 16, 16, 4));

  /* alignment */
  CHECK(sr_ptr_aligned((const void*)0x1000, 15) && sr_ptr_aligned((const void*)0x1010, 15));
  CHECK(!sr_ptr_aligned((const void*)0x1004, 15) && !sr_ptr_aligned((const void*)0x1008, 15));
  CHECK(sr_ptr_aligned((const void*)0x1008, 7) && !sr_ptr_aligned((const void*)0x1004, 7));
  CHECK(sr_ptr_aligned((const void*)0x1004, 3) && !sr_ptr_aligned((const void*)0x1002, 3));
  CHECK(sr_ptr_aligned((const void*)0, 15));
  CHECK(sr_rows_aligned((const void*)0x1000, 64 * 16, 16, 15, 4));
  CHECK(!sr_rows_aligned((const void*)0x1004, 64 * 16, 16, 15, 4));   /* pointer 4 bytes off */
  CHECK(!sr_rows_aligned((const void*)0x1000, 64 * 16, 18, 15, 4));   /* pixel stride C + 2 */
  CHECK(!sr_rows_aligned((const void*)0x1000, 64 * 16 + 2, 16, 15, 4));
  CHECK(sr_rows_aligned((const void*)0x1000, 0, 20, 15, 4));          /* a dense [M, C] view has no batch stride */
  CHECK(sr_rows_aligned((const void*)0x1008, 64 * 16, 16, 7, 4));     /* 16-bit tensors: 8-byte quads */
  CHECK(sr_rows_aligned((const void*)0x1000, 64 * 16, 24, 15, 8));    /* eight 16-bit channels per access */
  CHECK(!sr_rows_aligned((const void*)0x1000, 64 * 16, 20, 15, 8));
  CHECK(!sr_rows_aligned((const void*)0x1000, 64 * 16 + 4, 16, 15, 8));
  CHECK(sr_rows_aligned((const void*)0x1000, ((int64_t)1 << 40) + 4, 16, 15, 4));   /* a 64-bit batch stride is not truncated */
  CHECK(!sr_rows_aligned((const void*)0x1000, ((int64_t)1 << 40) + 2, 16, 15, 4));

  if (failures) return 1;
  printf("view checks ok\n");
  return 0;
}
