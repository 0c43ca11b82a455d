// The scalar arithmetic of the per-frame quality scores (include/dcunet.h, "Frame quality"; csrc/frame_quality.hip): the range of
// the three per-frame sums, the 128-bit numerators of a frame's correlation with a template, and the mean.  Plain C++ on top of
// footprint_math.h (dc_fp_corr is used unchanged), so the same inline functions compile for the device and into a stand-alone
// host program (tests/native/frame_math_check.cpp, run under the address / undefined-behaviour sanitizers).  No fused multiply-add
// and no reassociation anywhere: the pragma below, and -ffp-contract=off for frame_quality.hip in _build.py.
#pragma once
#pragma clang fp contract(off)
#include <stdint.h>

#include "footprint_math.h"

// Magnitudes.  A pixel and a template value are 16 bits: -32768 <= x <= 65535, so |x| < 2^16 and x^2, |x tmpl| <= 65535^2 < 2^32
// (ONE product needs 33 bits as a signed number: it is formed in 64).  The rectangle has n <= 2^28 pixels (DC_FRAME_MAX_PIXELS):
//   a = sum x          |a| <= 65535 n   <  2^44
//   b = sum x^2         b  <= 65535^2 n <  2^60
//   c = sum x tmpl     |c| <= 65535^2 n <  2^60             int64 holds all three, and so does every partial sum of them
//   an int32 partial of sum x is legal over a run of at most 32768 pixels (32768 * 65535 < 2^31); the kernel keeps none
//   n b < 2^88, a^2 < 2^88, so 0 <= Nxx < 2^88; |n c| < 2^88 and |a ta| < 2^88, so |Nxt| < 2^89; 0 <= Ntt < 2^88.
// Every intermediate stays far below 2^127, and the DcI128 operations, which wrap, never do.
#define DC_FRAME_MAX_PIXELS 268435456L                               /* 2^28 */

// the pixels of the rectangle [y0, y1) x [x0, x1) of an H x W frame, or -1 where it is empty or leaves the frame
DC_HD int64_t dc_frame_rect_pixels(int H, int W, int y0, int y1, int x0, int x1) {
  if (y0 < 0 || x0 < 0 || y1 > H || x1 > W || y0 >= y1 || x0 >= x1) return -1;
  return (int64_t)(y1 - y0) * (int64_t)(x1 - x0);
}

// {n b - a a, n c - a ta, n tb - ta ta}: n^2 times the variance of the frame, its covariance with the template and the
// template's variance over the rectangle -- the three numerators dc_fp_corr takes (frame, frame x template, template)
DC_HD DcFpNum dc_frame_numerators(int64_t n, int64_t a, int64_t b, int64_t c, int64_t ta, int64_t tb) {
  DcFpNum r;
  r.cxx = dc_i128_sub(dc_i128_mul(n, b), dc_i128_mul(a, a));
  r.cxl = dc_i128_sub(dc_i128_mul(n, c), dc_i128_mul(a, ta));
  r.cll = dc_i128_sub(dc_i128_mul(n, tb), dc_i128_mul(ta, ta));
  return r;
}

// both conversions are exact (|a| < 2^44, n <= 2^28): one rounding in the division, one to float32
DC_HD float dc_frame_mean(int64_t a, int64_t n) { return (float)((double)a / (double)n); }
