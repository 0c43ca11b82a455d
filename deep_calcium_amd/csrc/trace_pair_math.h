// The scalar arithmetic of the ROI trace-pair correlation (include/dcunet.h, "ROI trace-pair correlation"; csrc/trace_pairs.hip):
// the segment plan of a row of T sums, the term one segment adds to a numerator, and the range inside which every intermediate
// fits 128 bits.  Plain C++ on top of detrend_math.h, so the same inline functions compile for the device and into a stand-alone
// host program (tests/native/trace_pair_math_check.cpp, run under the address / undefined-behaviour sanitizers).  No fused
// multiply-add and no reassociation anywhere: the pragma below, and -ffp-contract=off for trace_pairs.hip in _build.py.
#pragma once
#pragma clang fp contract(off)
#include <stdint.h>

#include "detrend_math.h"

// Two rows x, y of int64 ROI sums over T frames, cut into the segments of detrend_math.h: n = max(1, T / L) segments, the last one
// absorbing the remainder, M = L * L_last (M = T when n == 1), mult_s = M / L_s.  With a_s = sum x, a'_s = sum y (int64) and
// g_s = sum x y (128 bits) over segment s,
//   N(x, y) = sum_s mult_s (L_s g_s - a_s a'_s)
// is dc_detrend_term_wide summed over the segments.
//
// Magnitudes.  Let B = floor(2^62 / max(M, T)) and |x|, |y| <= B for every value read (DC_TRACE_PAIR range: |S| max(M, T) <= 2^62).
// L_s <= T and L_s mult_s = M, so
//   |a_s|          <= L_s B            <= 2^62                      (int64)
//   |g_s|          <= L_s B^2          <= (T B) B <= 2^124          (128 bits: ONE product x y reaches 2^112 when |S| = 2^56)
//   |L_s g_s|      <= (L_s B)^2        <= 2^124
//   |a_s a'_s|     <= (L_s B)^2        <= 2^124
//   |mult_s L_s g_s| = M L_s B^2 = (M B)(L_s B) <= 2^124, and |mult_s a_s a'_s| <= the same: the two products
//   dc_detrend_term_wide forms before it subtracts; their difference is below 2^125.
//   The term itself is mult_s L_s^2 cov_s(x, y) with |cov_s| <= B^2 (Cauchy-Schwarz: cov^2 <= var x var y, and var <= B^2 for values
//   in [-B, B]), so |term_s| <= M L_s B^2 and |N| <= M T B^2 = (M B)(T B) <= 2^124; N(x, x) >= 0.
// With ROI sums, |S_i| <= 2^16 A_i for an ROI of A_i 16-bit pixels, and max(M, T) A <= 2^46 (the volume limits T H W <= 2^46 and
// M H W <= 2^46 with A <= H W) puts every value inside the range: |N| <= 2^32 (M A_i)(T A_j) <= 2^124 -- detrend_math.h's Css bound
// with A_i A_j in place of A^2; Cauchy-Schwarz gives the cross term.  Every intermediate stays below 2^127, and the DcI128
// operations, which wrap, never do.  The range is the CALLER'S promise, as |num| < 2^62 is for dc_trace_baseline.
#define DC_TRACE_PAIR_MAX_PAIRS 16777216L
#define DC_TRACE_PAIR_RANGE 4611686018427387904L                    /* 2^62 */

// n segments: n - 1 of L frames and a last one of `last` frames; one segment: L == last == T (also for T == 0)
struct DcTracePairPlan { int64_t n, L, last, M; };

// seg_len == 0: one segment of T frames.  Otherwise L = seg_len (the entry point has checked [2, 4096]).
DC_HD DcTracePairPlan dc_trace_pair_plan(int64_t T, int64_t seg_len) {
  DcTracePairPlan p;
  p.n = seg_len > 0 ? T / seg_len : 1;
  if (p.n <= 1) {
    p.n = 1; p.L = T; p.last = T; p.M = T;
  } else {
    p.L = seg_len;
    p.last = T - (p.n - 1) * seg_len;
    p.M = p.L * p.last;
  }
  return p;
}

// segment s in [0, n): where it starts, how long it is, and mult = M / len
DC_HD void dc_trace_pair_segment(DcTracePairPlan p, int64_t s, int64_t* start, int64_t* len, int64_t* mult) {
  *start = s * p.L;
  if (p.n == 1) { *len = p.last; *mult = 1; }
  else if (s < p.n - 1) { *len = p.L; *mult = p.last; }
  else { *len = p.last; *mult = p.L; }
}

// |v| * max(M, T) <= 2^62, without overflow (INT64_MIN is outside for every plan)
DC_HD bool dc_trace_pair_range_ok(int64_t v, DcTracePairPlan p, int64_t T) {
  const int64_t m = p.M > T ? p.M : T;
  if (m <= 0) return true;
  const int64_t lim = DC_TRACE_PAIR_RANGE / m;
  return v >= -lim && v <= lim;
}

// mult * (len * g - a * a2) with a 128-bit g: what one segment adds to N(x, y)
DC_HD DcI128 dc_trace_pair_term(int64_t len, int64_t mult, DcI128 g, int64_t a, int64_t a2) {
  return dc_detrend_term_wide(len, mult, g, a, a2);
}
