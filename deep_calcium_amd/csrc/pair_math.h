// The scalar arithmetic of the ROI pixel-pair correlation (include/dcunet.h, "ROI pixel-pair correlation"; csrc/roi_pairs.hip)
// beyond footprint_math.h: the three numerators of one pair from the exact integer moments, in the form dc_fp_corr takes, and
// the bookkeeping of the tiles of an ROI's square.  Plain C++ like footprint_math.h, so the same inline functions compile for the
// device and into a stand-alone host program (tests/native/pair_math_check.cpp, run under the address / undefined-behaviour
// sanitizers).  No fused multiply-add and no reassociation anywhere: the pragma below, and -ffp-contract=off for roi_pairs.hip.
#pragma once
#pragma clang fp contract(off)
#include <stdint.h>

#include "footprint_math.h"

// Magnitudes.  |x| < 2^16 and T <= 2^31 - 1 (DC_FP_MAX_FRAMES):
//   a_i  = sum x_i        |a|  <  2^16 T          <  2^47
//   g_ij = sum x_i x_j    |g|  <= 65535^2 T       <  2^63       (int64; ONE product needs 33 bits: 65535^2 > 2^31)
//   T g_ij                |.|  <  2^31 2^63       =  2^94
//   a_i a_j               |.|  <  2^94
//   Cij = T g_ij - a_i a_j     |Cij| < 2^95, and Cii = T^2 var(x_i) >= 0, Cij^2 <= Cii Cjj (Cauchy-Schwarz, exact integers).
// Every intermediate stays far below 2^127, and the DcI128 operations, which wrap, never do.

// {cxx, cxl, cll} = {Cii, Cij, Cjj}: dc_fp_corr of it is corr(x_i, x_j).  The product sqrt(f64(Cii)) * sqrt(f64(Cjj)) commutes, so
// corr_ij and corr_ji are the same bits; for i == j the three numerators are one integer and the quotient rounds to 1.0f.
DC_HD DcFpNum dc_pair_numerators(int64_t T, int64_t ai, int64_t aj, int64_t gii, int64_t gij, int64_t gjj) {
  DcFpNum n;
  n.cxx = dc_i128_sub(dc_i128_mul(T, gii), dc_i128_mul(ai, ai));
  n.cxl = dc_i128_sub(dc_i128_mul(T, gij), dc_i128_mul(ai, aj));
  n.cll = dc_i128_sub(dc_i128_mul(T, gjj), dc_i128_mul(aj, aj));
  return n;
}

// The tiles (ti, tj), ti <= tj, of a k x k square cut into tiles of edge `tile`: nt (nt + 1) / 2 with nt = ceil(k / tile).
DC_HD int64_t dc_pair_tiles_of(int64_t k, int64_t tile) {
  const int64_t nt = (k + tile - 1) / tile;
  return nt * (nt + 1) / 2;
}

// Does ROI [p0, p1) of a state of P pixels and G words, with its square at go, lie inside the state and the limits?  What both
// kernels ask before they touch anything: an ROI that fails is skipped whole.
DC_HD bool dc_pair_roi_ok(int64_t p0, int64_t p1, int64_t go, int64_t P, int64_t G, int64_t max_area) {
  if (p0 < 0 || p1 > P || p1 <= p0) return false;
  const int64_t k = p1 - p0;
  if (k > max_area) return false;
  return go >= 0 && go <= G - k * k;                 // k <= max_area: k * k cannot overflow
}
