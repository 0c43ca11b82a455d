// The scalar arithmetic of the ROI footprint maps (include/dcunet.h, "ROI footprint maps"; csrc/footprints.hip): the split of an
// ROI sum into two 32-bit words whose products with a pixel can be summed in int64, the fold of those sums into the 128-bit
// moment, and the correlation of one support entry from its exact integer moments.  Plain C++ like dff_math.h, on top of
// series_math.h, so the same inline functions compile for the device and into a stand-alone host program
// (tests/native/footprint_math_check.cpp, run under the address / undefined-behaviour sanitizers).  No fused multiply-add and no
// reassociation anywhere: the pragma below, and -ffp-contract=off for footprints.hip in _build.py.
#pragma once
#pragma clang fp contract(off)
#include <math.h>
#include <stdint.h>

#include "series_math.h"

// Magnitudes.  A pixel is 16 bits, |x| < 2^16; an ROI has A <= H * W pixels, so |S| <= 2^16 A; the limits are
// T * H * W <= 2^46 (DC_ROI_TRACE_MAX_VOLUME) and T <= 2^31 - 1 (DC_ROI_PIXEL_MAX_FRAMES), hence T A <= 2^46.
//   a = sum x        |a| <  2^16 T        <  2^47
//   b = sum x^2       b  <  2^32 T        <  2^63       (why T is limited to 2^31 - 1: b is an int64)
//   c = sum x S      |c| <= 2^32 T A      <= 2^78       (128 bits)
//   u = sum S        |u| <= 2^16 T A      <= 2^62
//   w = sum S^2       w  <= 2^32 T A^2                  (128 bits)
//   T b < 2^94, a^2 < 2^94, so 0 <= Cxx < 2^94;
//   |T c| <= 2^32 (T A) T < 2^109, |a u| < 2^47 2^62 = 2^109, so |Cxs| < 2^110;
//   T w <= 2^32 (T A)^2 <= 2^124, u^2 <= 2^124, and both are >= 0 with T w >= u^2, so 0 <= Css <= 2^124;
//   Cxl = Cxs - Cxx: below 2^111.  Cll = Css - 2 Cxs + Cxx = T^2 var(S - x) with |S - x| <= 2^16 A (the pixel is one of the
//   ROI's): 0 <= Cll <= T^2 (2^16 A)^2 <= 2^124, and its partial sum |Css - 2 Cxs| < 2^124 + 2^111 < 2^125.
// Every intermediate therefore stays below 2^127, and the DcI128 operations, which wrap, never do.
#define DC_FP_MAX_FRAMES 2147483647L

// S = hi * 2^32 + lo with 0 <= lo < 2^32: exact for every int64 (the shift of a negative value is arithmetic).
DC_HD void dc_fp_split(int64_t s, uint32_t* lo, int32_t* hi) {
  *lo = (uint32_t)((uint64_t)s & 0xffffffffull);
  *hi = (int32_t)(s >> 32);
}

// c + acc_lo + acc_hi * 2^32, where acc_lo = sum x * S_lo and acc_hi = sum x * S_hi over a bounded run of frames
DC_HD DcI128 dc_fp_fold(DcI128 c, int64_t acc_lo, int64_t acc_hi) {
  DcI128 h;
  h.lo = (uint64_t)acc_hi << 32;
  h.hi = acc_hi >> 32;                               // arithmetic: the sign goes with it
  return dc_i128_add(dc_i128_add(c, dc_i128_from_i64(acc_lo)), h);
}

DC_HD bool dc_i128_is_positive(DcI128 a) { return a.hi > 0 || (a.hi == 0 && a.lo != 0); }

// The three numerators of one entry.  T frames; a, b, c the entry's moments; u, w its ROI's; inside: the pixel is one of the
// ROI's and is taken out of the trace it is compared with (L = S - x).
struct DcFpNum { DcI128 cxx, cxl, cll; };

DC_HD DcFpNum dc_fp_numerators(int64_t T, int64_t a, int64_t b, DcI128 c, int64_t u, DcI128 w, bool inside) {
  DcFpNum n;
  n.cxx = dc_i128_sub(dc_i128_mul(T, b), dc_i128_mul(a, a));
  const DcI128 cxs = dc_i128_sub(dc_i128_mul_i64(c, T), dc_i128_mul(a, u));
  const DcI128 css = dc_i128_sub(dc_i128_mul_i64(w, T), dc_i128_mul(u, u));
  if (inside) {
    n.cxl = dc_i128_sub(cxs, n.cxx);
    n.cll = dc_i128_add(dc_i128_sub(css, dc_i128_add(cxs, cxs)), n.cxx);
  } else {
    n.cxl = cxs;
    n.cll = css;
  }
  return n;
}

// corr = (float)(f64(Cxl) / (sqrt(f64(Cxx)) * sqrt(f64(Cll)))), one rounding per numerator; exactly 0 where Cxx <= 0 or Cll <= 0
// (a pixel or a trace that is constant in time, T == 1, the pixel of a one-pixel ROI): numpy gives NaN there.
DC_HD float dc_fp_corr(DcFpNum n) {
  if (!dc_i128_is_positive(n.cxx) || !dc_i128_is_positive(n.cll)) return 0.f;
  const double den = sqrt(dc_i128_to_f64(n.cxx)) * sqrt(dc_i128_to_f64(n.cll));
  return (float)(dc_i128_to_f64(n.cxl) / den);
}
