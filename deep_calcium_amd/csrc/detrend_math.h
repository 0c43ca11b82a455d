// The scalar arithmetic of the detrended (segment-pooled) correlations (include/dcunet.h, "Detrended correlations";
// csrc/series.hip, csrc/roi_pairs.hip, csrc/footprints.hip): the term one segment adds to a pooled numerator, the limits of a
// segment, and the footprint rule on pooled numerators.  Plain C++ on top of pair_math.h, so the same inline functions compile for
// the device and into a stand-alone host program (tests/native/detrend_math_check.cpp, run under the address / undefined-behaviour
// sanitizers).  No fused multiply-add and no reassociation anywhere: the pragma below, and -ffp-contract=off for the three files.
#pragma once
#pragma clang fp contract(off)
#include <stdint.h>

#include "pair_math.h"

// The T frames a reader sees are cut into n = max(1, T / L) segments: n - 1 of L frames and a last one of L_last = T - (n - 1) L
// frames, L <= L_last < 2 L; one segment of T frames when T < 2 L.  M = L * L_last (M = T when n == 1) and mult_s = M / L_s, so
// for EVERY segment len * mult == M.  For two series x, y with per-segment sums a = sum x, a' = sum y, g = sum x y
//   N(x, y) = sum_s mult_s (L_s g_s - a_s a'_s)  =  M * (the within-segment centred cross sum, pooled over the segments)
// is an exact integer, and with n == 1 it is today's T g - a a'.
//
// Magnitudes.  |x| < 2^16, L <= 4096 = DC_DETREND_MAX_FRAMES, so in a recording of several segments len <= 8191, mult <= 8191 and
// M < 2^25; with one segment len = T <= 2^31 - 1 and mult = 1.  In both cases M <= 2^31 and T <= 2^31 - 1.
//   pixel with pixel (series, pairs):  g_s <= 65535^2 L_s (int64 for any L_s <= 2^31 - 1), |L_s g_s|, |a_s a'_s| < 2^32 L_s^2 <= 2^94,
//     the segment's term |mult_s (L_s g_s - a_s a'_s)| <= 2^32 M L_s, and the pooled sum |N| <= 2^32 M T < 2^95.
//   footprints, A <= H * W pixels per ROI, |S| <= 2^16 A, under T * H * W <= 2^46 AND M * H * W <= 2^46 (DC_DETREND_MAX_VOLUME):
//     c_s = sum x S:  |L_s c_s| <= 2^32 L_s^2 A, |a_s u_s| <= the same, so |mult_s (L_s c_s - a_s u_s)| <= 2^33 M L_s A and
//       |Cxs| <= 2^33 (M A) T <= 2^33 2^46 2^31 = 2^110;
//     w_s = sum S^2:  L_s w_s <= 2^32 L_s^2 A^2 and u_s^2 <= the same with L_s w_s >= u_s^2 (Cauchy-Schwarz), so the term lies in
//       [0, 2^32 M L_s A^2] and 0 <= Css <= 2^32 (M A) (T A) <= 2^124: footprint_math.h's bound with M in place of one factor T;
//       the product mult_s * (L_s w_s), formed before the subtraction, obeys the same bound.
//     inside entries: Cxl = Cxs - Cxx below 2^111; Cll = Css - 2 Cxs + Cxx = M * (the pooled centred sum of squares of S - x), with
//       |S - x| <= 2^16 A: 0 <= Cll <= 2^124, and the partial sum |Css - 2 Cxs| < 2^124 + 2^111 < 2^125.
// Every intermediate therefore stays below 2^127, and the DcI128 operations, which wrap, never do.
#define DC_DETREND_MIN_FRAMES 2
#define DC_DETREND_MAX_FRAMES 4096
#define DC_DETREND_MAX_SEGMENT (2 * DC_DETREND_MAX_FRAMES - 1)      /* L_last < 2 L: the longest segment beside another one, and the largest mult */
#define DC_DETREND_MAX_VOLUME 70368744177664L                        /* M * H * W <= 2^46 */

// Is (len, mult) a segment the fold kernels can take?  One segment alone (mult == 1) may be as long as the recording; a segment
// beside others is at most DC_DETREND_MAX_SEGMENT frames and so is its mult.
DC_HD bool dc_detrend_segment_ok(int64_t len, int64_t mult) {
  if (len < 1 || mult < 1 || len > DC_FP_MAX_FRAMES) return false;
  return mult == 1 || (len <= DC_DETREND_MAX_SEGMENT && mult <= DC_DETREND_MAX_SEGMENT);
}

// M = len * mult of an accepted segment times `area` (H * W) against DC_DETREND_MAX_VOLUME, without overflow: M <= 2^31, area <= 2^30
DC_HD bool dc_detrend_volume_ok(int64_t len, int64_t mult, int64_t area) {
  return area >= 0 && area <= ((int64_t)1 << 30) && len * mult <= DC_DETREND_MAX_VOLUME / (area > 0 ? area : 1);
}

// mult * (len * g - a * a2): what one segment adds to the pooled numerator of two 16-bit series
DC_HD DcI128 dc_detrend_term(int64_t len, int64_t mult, int64_t g, int64_t a, int64_t a2) {
  return dc_i128_mul_i64(dc_i128_sub(dc_i128_mul(len, g), dc_i128_mul(a, a2)), mult);
}

// the same with a 128-bit cross sum: c = sum x S against a = sum x, u = sum S; and w = sum S^2 against u twice.  The factors are
// applied one after the other to the cross sum (mult * len * c never leaves the bound of the header) so that no 128 x 128 product
// is needed.
DC_HD DcI128 dc_detrend_term_wide(int64_t len, int64_t mult, DcI128 c, int64_t a, int64_t u) {
  return dc_i128_sub(dc_i128_mul_i64(dc_i128_mul_i64(c, len), mult), dc_i128_mul_i64(dc_i128_mul(a, u), mult));
}

// The three numerators of one support entry from the POOLED Cxx, Cxs of the entry and Css of its ROI: the rule of
// dc_fp_numerators is linear in the moments, so it holds segment by segment and therefore for the pooled sums.
DC_HD DcFpNum dc_detrend_fp_numerators(DcI128 cxx, DcI128 cxs, DcI128 css, bool inside) {
  DcFpNum n;
  n.cxx = cxx;
  if (inside) {
    n.cxl = dc_i128_sub(cxs, cxx);
    n.cll = dc_i128_add(dc_i128_sub(css, dc_i128_add(cxs, cxs)), cxx);
  } else {
    n.cxl = cxs;
    n.cll = css;
  }
  return n;
}

// std = sqrt(f64(N(x, x)) / f64(M * T)): the population standard deviation of the detrended series, one rounding of the numerator,
// one of M * T (an int64 below 2^62), a divide and a square root in double: within 1 float32 ulp of the exact value.
DC_HD double dc_detrend_var(DcI128 nxx, int64_t M, int64_t T) { return dc_i128_to_f64(nxx) / (double)(M * T); }

#if defined(__HIPCC__)
// A pooled word is one 16-byte {lo, hi} element: one 16-byte load, one 16-byte store.
__device__ __forceinline__ DcI128 dc_i128_load(const int64_t* p, long i) {
  const ulonglong2 v = reinterpret_cast<const ulonglong2*>(p)[i];
  DcI128 r;
  r.lo = v.x;
  r.hi = (int64_t)v.y;
  return r;
}
__device__ __forceinline__ void dc_i128_store(int64_t* p, long i, DcI128 v) {
  ulonglong2 w;
  w.x = v.lo;
  w.y = (uint64_t)v.hi;
  reinterpret_cast<ulonglong2*>(p)[i] = w;
}
#endif
