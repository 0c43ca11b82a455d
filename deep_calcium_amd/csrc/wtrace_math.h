// The scalar arithmetic of the weighted ROI sums (include/dcunet.h, "Weighted ROI traces"; the WGT form of the accumulate kernel in
// csrc/traces.hip): one term w x, what 32 bits can and cannot hold of it, and the ranges the unchanged finalize, baseline and
// trace-pair entry points are promised when the weight sum W stands where the area stood.  Plain integer C++, so the same inline
// functions compile for the device and into a stand-alone host program (tests/native/wtrace_math_check.cpp, run under the address /
// undefined-behaviour sanitizers).  There is no floating point here.
#pragma once
#include <stdint.h>

#ifndef DC_HD
#ifdef __HIPCC__
#define DC_HD __host__ __device__ inline
#else
#define DC_HD inline
#endif
#endif

// Magnitudes.  A weight is any uint16: 0 <= w <= 65535.  A pixel is 16 bits: -32768 <= x <= 32767 (int16) or 0 <= x <= 65535.
//   one term w x      int16 frames:  |w x| <= 65535 * 32768 = 2^31 - 32768   -- fits int32, with room for nothing else:
//                                    two terms reach 2^32 - 65536 > 2^31 - 1
//                     uint16 frames:  w x  <= 65535^2 = 2^32 - 131071         -- does not fit int32 at all
//   so NO partial sum of terms may be held in 32 bits, not even a lane's share of one piece (32 terms): where the unweighted kernel
//   keeps int32 over a piece (2048 * 65535 < 2^27), the weighted one forms the term by a 32 x 32 -> 64-bit multiply-add
//   (v_mad_i64_i32: w and x are both int32 in range) and sums in int64 from the first term on.
//   a row of n entries: |sum| <= n (2^32 - 131071); n <= 2^30 entries per ROI (DC_WTRACE_MAX_ENTRIES, H W <= 2^30 and an ROI lists a
//   pixel at most once; duplicates count towards n) keep |S| < 2^62, and every partial sum of any subset, in any order, is bounded
//   by the same figure: lanes, waves, rows and the atomics into a zeroed column cannot overflow int64 on the way.
// Downstream (dc_roi_trace_finalize, dc_trace_baseline*, dc_trace_pair_*) an "area" A is an int32 divisor with |S| <= 65535 A and
// T A <= 2^46.  With A = W = sum of w over the ROI: |S| = |sum w x| <= 65535 sum w = 65535 W holds term by term, so the caller
// only has to keep 1 <= W <= 2^31 - 1 and T W <= 2^46 (DC_WTRACE_MAX_VOLUME).
#define DC_WTRACE_MAX_WEIGHT 65535
#define DC_WTRACE_MAX_ENTRIES 1073741824L                            /* 2^30 */
#define DC_WTRACE_MAX_WSUM 2147483647L                               /* 2^31 - 1: W is handed on as an int32 "area" */
#define DC_WTRACE_MAX_VOLUME 70368744177664L                         /* 2^46 = DC_ROI_TRACE_MAX_VOLUME, here T * W */

// w x, exact: both factors are int32 in range, the product is formed in 64 bits
DC_HD int64_t dc_wtrace_term(int w, int x) { return (int64_t)w * (int64_t)x; }

// the largest |S| a row of n entries can reach (both frame types): n * 65535^2
DC_HD int64_t dc_wtrace_row_bound(int64_t n) { return n * ((int64_t)DC_WTRACE_MAX_WEIGHT * DC_WTRACE_MAX_WEIGHT); }

// how many terms of the worst case an int32 partial sum survives: 1 for int16 frames, 0 for uint16 frames
DC_HD int dc_wtrace_int32_terms(int is_unsigned) {
  const int64_t term = is_unsigned ? (int64_t)65535 * 65535 : (int64_t)65535 * 32768;
  return (int)(2147483647L / term);
}

// 0 where W can stand for an area over T frames, else which promise breaks: 1 = W < 1, 2 = W > 2^31 - 1, 3 = T W > 2^46
DC_HD int dc_wtrace_wsum_check(int64_t wsum, int64_t T) {
  if (wsum < 1) return 1;
  if (wsum > DC_WTRACE_MAX_WSUM) return 2;
  if (T > 0 && wsum > DC_WTRACE_MAX_VOLUME / T) return 3;
  return 0;
}
