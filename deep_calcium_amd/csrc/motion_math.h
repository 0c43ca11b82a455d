// The tie rule of rigid motion correction (motion.hip, dc_motion_pick): among the candidate shifts (dy, dx) of one frame the picked
// one minimises the tuple (score, dy^2 + dx^2, dy, dx) lexicographically -- the smallest sum of squared differences, then the
// smallest displacement, then the smaller dy, then the smaller dx.  Two candidates with different (dy, dx) never compare equal, so
// the minimum is unique and does not depend on the order in which candidates are compared.  Plain C++ on purpose -- no HIP header,
// no intrinsic -- so the same inline functions compile for the device and into a stand-alone host program
// (tests/native/motion_math_check.cpp, run under the address / undefined-behaviour sanitizers).  Below the tie rule: the block
// geometry and the shift field of the piecewise-rigid mode (tests/native/motion_field_check.cpp), in the same plain C++.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DC_MOTION_HD __host__ __device__ inline
#else
#define DC_MOTION_HD inline
#endif

struct DcShiftCand {
  int64_t score;
  int dy, dx;
};

// |dy|, |dx| <= 16 in dc_motion_pick; any int32 pair is ordered correctly (each square is <= 2^62, their sum fits 64 unsigned bits)
DC_MOTION_HD uint64_t dc_motion_dist2(int dy, int dx) { return (uint64_t)((int64_t)dy * dy) + (uint64_t)((int64_t)dx * dx); }

// true when a comes strictly before b in the order above
DC_MOTION_HD bool dc_motion_before(const DcShiftCand a, const DcShiftCand b) {
  if (a.score != b.score) return a.score < b.score;
  const uint64_t da = dc_motion_dist2(a.dy, a.dx), db = dc_motion_dist2(b.dy, b.dx);
  if (da != db) return da < db;
  if (a.dy != b.dy) return a.dy < b.dy;
  return a.dx < b.dx;
}

// candidate i of the [2S+1][2S+1] score table of one frame (dy the slow axis, index dy + S)
DC_MOTION_HD DcShiftCand dc_motion_cand(const int64_t* scores, int S, int i) {
  const int nd = 2 * S + 1;
  DcShiftCand c;
  c.score = scores[i];
  c.dy = i / nd - S;
  c.dx = i % nd - S;
  return c;
}

// the picked shift of one frame: a serial scan (what the kernel's strided scan + wave reduction must equal)
DC_MOTION_HD DcShiftCand dc_motion_pick_serial(const int64_t* scores, int S) {
  const int nd = 2 * S + 1;
  DcShiftCand best = dc_motion_cand(scores, S, 0);
  for (int i = 1; i < nd * nd; ++i) {
    const DcShiftCand c = dc_motion_cand(scores, S, i);
    if (dc_motion_before(c, best)) best = c;
  }
  return best;
}

// ---- piecewise-rigid correction (motion.hip, dc_motion_block_ssd / dc_motion_warp): block geometry and the shift field, integers only ---------------------------
// An axis of n pixels is cut into B blocks; block i covers [e(i), e(i+1)) with e(i) = floor(i * n / B).  n <= 2^30, B <= 32.
DC_MOTION_HD int dc_block_edge(int i, int n, int B) { return (int)((int64_t)i * n / B); }

// every block clipped to the interior [M, n - M) keeps a pixel: the first and the last one do (the others lie between them)
DC_MOTION_HD bool dc_block_axis_ok(int n, int B, int M) {
  if (B < 1 || n < B || M < 0 || n <= 2 * (int64_t)M) return false;
  const int first = dc_block_edge(1, n, B) < n - M ? dc_block_edge(1, n, B) : n - M;
  const int last = dc_block_edge(B - 1, n, B) > M ? dc_block_edge(B - 1, n, B) : M;
  return first > M && last < n - M;
}

// Where pixel y stands between the block centres, in doubled coordinates p = 2y and C2(i) = e(i) + e(i+1) - 1 (strictly increasing
// when every block has a pixel, n >= B): at or before the first centre (or B == 1) i0 = i1 = 0, at or after the last i0 = i1 =
// B - 1, both with w = 0; otherwise i0 is the largest i with C2(i) <= p, i1 = i0 + 1 and
// w = floor(256 * (p - C2(i0)) / (C2(i1) - C2(i0))) in [0, 256).  The block b that holds y has C2(b - 1) < p < C2(b + 1), so i0 is
// b or b - 1: no search over the centres.
struct DcFieldTap {
  int i0, i1, w;
};

// The tap from a table of the edges e[0 .. B] (the warp kernel keeps one per axis in LDS): no division but the one for w, and that
// one in 32 bits where the numerator fits.  The block that holds y is found by bisection (e is strictly increasing).
DC_MOTION_HD DcFieldTap dc_field_tap_edges(int y, const int* e, int B) {
  DcFieldTap t;
  t.i0 = t.i1 = t.w = 0;
  const int64_t p = 2 * (int64_t)y;
  if (B == 1 || p <= (int64_t)e[0] + e[1] - 1) return t;
  if (p >= (int64_t)e[B - 1] + e[B] - 1) {
    t.i0 = t.i1 = B - 1;
    return t;
  }
  int lo = 0, hi = B - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) / 2;
    if (e[mid] <= y) lo = mid; else hi = mid - 1;
  }
  t.i0 = p >= (int64_t)e[lo] + e[lo + 1] - 1 ? lo : lo - 1;
  t.i1 = t.i0 + 1;
  const int64_t c0 = (int64_t)e[t.i0] + e[t.i0 + 1] - 1, c1 = (int64_t)e[t.i1] + e[t.i1 + 1] - 1;
  if (c1 - c0 < (1 << 23)) t.w = (int)((uint32_t)(256 * (p - c0)) / (uint32_t)(c1 - c0));      // the numerator is below 2^31
  else t.w = (int)(256 * (p - c0) / (c1 - c0));
  return t;
}

// floor(a / 65536) for any sign
DC_MOTION_HD int64_t dc_floor_div_65536(int64_t a) {
  const int64_t q = a / 65536;
  return (a % 65536 < 0) ? q - 1 : q;
}

// One axis of the bilinear blend: (256 - w) * s0 + w * s1, exact for any int32 s0, s1 (below 2^40 in magnitude)
DC_MOTION_HD int64_t dc_field_blend(int64_t s0, int64_t s1, int w) { return (256 - w) * s0 + w * s1; }

// The field from the four block shifts around a pixel:
//   num = (256-w) * ((256-v) * s00 + v * s01) + w * ((256-v) * s10 + v * s11),  field = floor((num + 32768) / 65536).
// |num| <= 2^16 * 2^31: 64 bits hold it.  The field lies in [min s, max s]; equal shifts give that shift.
DC_MOTION_HD int64_t dc_field_value(int64_t s00, int64_t s01, int64_t s10, int64_t s11, int w, int v) {
  return dc_floor_div_65536(dc_field_blend(dc_field_blend(s00, s01, v), dc_field_blend(s10, s11, v), w) + 32768);
}

// the same from the two row blends a0 = blend(s00, s10, w), a1 = blend(s01, s11, w): the sum is the same integer in either order
DC_MOTION_HD int64_t dc_field_from_rows(int64_t a0, int64_t a1, int v) { return dc_floor_div_65536(dc_field_blend(a0, a1, v) + 32768); }

// ... and from a0 and the difference d = a1 - a0 where |d| < 2^22 (block shifts less than 2^14 pixels apart): (256-v) a0 + v a1 =
// 256 a0 + v d, and v d fits 32 bits -- one 24-bit multiplication per pixel instead of two 64-bit ones
DC_MOTION_HD bool dc_field_delta_small(int64_t d) { return d > -(1 << 22) && d < (1 << 22); }
DC_MOTION_HD int64_t dc_field_from_delta(int64_t a0, int d, int v) { return dc_floor_div_65536(256 * a0 + (int64_t)(v * d) + 32768); }

DC_MOTION_HD int dc_motion_clamp(int v, int S) { return v < -S ? -S : (v > S ? S : v); }

// ---- sub-pixel correction (motion.hip, dc_motion_refine / dc_motion_apply_sub / dc_motion_warp_sub): FINE shifts, int32 in units of
// 1 / DC_MOTION_SUB of a pixel, same sign convention; 16 dy is exactly the whole-pixel shift dy.  Integers only.
// (tests/native/motion_sub_check.cpp)
#ifndef DC_MOTION_SUB
#define DC_MOTION_SUB 16                 // include/dcunet.h defines the same value
#endif

// One axis of the refinement of a pick: s0 the picked score, sm and sp its neighbours at -1 and +1 on that axis.  The vertex of the
// parabola through the three lies at N / (2 D) pixels from the pick, N = sm - sp, D = sm - 2 s0 + sp; in sixteenths, rounded to
// the nearest with a tie at a half going to the pick:
//   D == 0: q = 0;  otherwise m = floor((16 |N| + D - 1) / (2 D)),  q = sign(N) * m.
// s0 is the minimum of the three, so D >= 0 and |N| <= D: q lies in [-8, 8].  A symmetric neighbourhood (sm == sp) gives 0,
// sm == s0 < sp gives exactly -8, swapping sm and sp negates q (the mirror image of a table gives the mirrored q), and N = 1,
// D = 16 -- half a sixteenth -- gives 0.
// Scores go up to 2^62 - 1, so 16 |N| does not fit 64 bits and is never formed: 16 |N| = t D + r with 0 <= r < D comes from four
// doubling steps of a long division (every intermediate is below 2 D <= 2^64 - 4), and then
//   m = floor(((t + 1) D + r - 1) / (2 D)) = floor((t + 1) / 2) where r > 0, floor(t / 2) where r == 0.
// Scores that are not those of a pick (s0 not the minimum; only a caller's own table can hold them) stay defined: D <= 0 gives 0,
// |N| >= D gives +-8, and the differences wrap like unsigned arithmetic.
DC_MOTION_HD int dc_motion_subpixel(int64_t sm, int64_t s0, int64_t sp) {
  const int64_t N = (int64_t)((uint64_t)sm - (uint64_t)sp);
  const int64_t D = (int64_t)(((uint64_t)sm - (uint64_t)s0) + ((uint64_t)sp - (uint64_t)s0));
  if (D <= 0 || N == 0) return 0;
  const uint64_t a = N < 0 ? 0ull - (uint64_t)N : (uint64_t)N, d = (uint64_t)D;
  int m = DC_MOTION_SUB / 2;
  if (a < d) {
    uint64_t r = a;
    int t = 0;
    for (int i = 0; i < 4; ++i) {                        // 16 = 2^4
      r <<= 1;
      t <<= 1;
      if (r >= d) { r -= d; t += 1; }
    }
    m = r ? (t + 1) / 2 : t / 2;
  }
  return N < 0 ? -m : m;
}

// (qy, qx) of the entry (py, px) of one [2R+1][2R+1] score table (py the slow axis, index py + R): per axis dc_motion_subpixel of
// the entry and its two neighbours on that axis, the other axis held; 0 on an axis where the entry lies on the table's border.  An
// entry outside [-R, R]^2 gives (0, 0) and reads nothing.
struct DcSubShift {
  int qy, qx;
};
DC_MOTION_HD DcSubShift dc_motion_refine_entry(const int64_t* table, int R, int py, int px) {
  DcSubShift q;
  q.qy = q.qx = 0;
  if (py < -R || py > R || px < -R || px > R) return q;
  const int nd = 2 * R + 1;
  const int64_t* c = table + (py + R) * nd + (px + R);
  if (py > -R && py < R) q.qy = dc_motion_subpixel(c[-nd], c[0], c[nd]);
  if (px > -R && px < R) q.qx = dc_motion_subpixel(c[-1], c[0], c[1]);
  return q;
}

// 16 * whole + q in wrapping 32-bit arithmetic (exact for |whole| < 2^27, which every searched shift is)
DC_MOTION_HD int dc_motion_fine(int whole, int q) { return (int)((uint32_t)whole * (uint32_t)DC_MOTION_SUB + (uint32_t)q); }

// The split of a fine shift s: i = floor(s / 16), f = s - 16 i in [0, 16), for either sign
DC_MOTION_HD int dc_motion_floor16(int s) {
  const int q = s / DC_MOTION_SUB;
  return (s % DC_MOTION_SUB < 0) ? q - 1 : q;
}
DC_MOTION_HD int dc_motion_frac16(int s) { return (int)((int64_t)s - (int64_t)DC_MOTION_SUB * dc_motion_floor16(s)); }

// Bilinear interpolation between four taps a_ij = frame[y + iy + i][x + ix + j], any values in [-32768, 65535]:
//   out = floor(((16-fy) ((16-fx) a00 + fx a01) + fy ((16-fx) a10 + fx a11) + 128) / 256).
// The weights are non-negative and add up to 256, so out lies between the smallest and the largest tap (it fits their dtype), equal
// taps give that value, and adding a constant to all four adds it to out -- the kernels interpolate int16 values with the sign bit
// flipped.  |numerator| < 2^25; the floor for either sign comes from shifting a numerator made positive by 2^15 * 256.
DC_MOTION_HD int dc_motion_interp(int a00, int a01, int a10, int a11, int fy, int fx) {
  const int gx = DC_MOTION_SUB - fx, gy = DC_MOTION_SUB - fy;
  const int num = gy * (gx * a00 + fx * a01) + fy * (gx * a10 + fx * a11) + 128;
  return ((num + (1 << 23)) >> 8) - (1 << 15);
}

// ---- wide search (motion.hip, dc_motion_bin / dc_motion_ssd_around / dc_motion_pick_around): a coarse pick on frames binned c x c,
// then the scores of the full-resolution shifts within +-D of c times that pick.  Integers only.  (tests/native/motion_wide_check.cpp)
#ifndef DC_MOTION_MAX_WIDE_SHIFT
#define DC_MOTION_MAX_WIDE_SHIFT 128     // include/dcunet.h defines the same value
#endif

// log2 of the binning factor c, -1 where c is not one of 2, 4, 8
DC_MOTION_HD int dc_motion_bin_log2(int c) { return c == 2 ? 1 : (c == 4 ? 2 : (c == 8 ? 3 : -1)); }

// The value of one bin from the sum of its c x c = 4^lg cells (16-bit values, signed or unsigned: |sum| <= 64 * 65535):
// floor((sum + c^2 / 2) / c^2), the mean rounded half up -- the rule of the rounded-mean template.  The floor for a negative sum is
// spelled out (a right shift of a negative value is the compiler's choice before C++20).  The result lies between the smallest
// and the largest cell, so it fits their dtype.
DC_MOTION_HD int dc_motion_bin_round(int sum, int lg) {
  const int k = 2 * lg, a = sum + (1 << (k - 1));
  return a >= 0 ? a >> k : -((-a + (1 << k) - 1) >> k);
}

// The centre of a frame's fine window on one axis: clamp(mult * row, -M, M), M = S - D >= 0.  The product is formed in 64 bits, so
// any int32 row (and any int32 mult) is legal; centre + [-D, D] lies inside [-S, S].
DC_MOTION_HD int dc_motion_centre(int mult, int row, int M) {
  const int64_t v = (int64_t)mult * row;
  return v < -(int64_t)M ? -M : (v > (int64_t)M ? M : (int)v);
}

// candidate i of the [2D+1][2D+1] window table of one frame (ey the slow axis, index ey + D) as the TOTAL shift centre + (ey, ex):
// the order of dc_motion_before is then over total shifts, so the pick equals the exhaustive pick of radius S whenever that
// pick lies inside the window -- an order over the residuals would prefer the candidate nearest the centre instead.
DC_MOTION_HD DcShiftCand dc_motion_cand_around(const int64_t* wscores, int D, int i, int cy, int cx) {
  DcShiftCand c = dc_motion_cand(wscores, D, i);
  c.dy += cy;
  c.dx += cx;
  return c;
}

// the picked total shift of one frame: a serial scan (what the kernel's strided scan + wave reduction must equal)
DC_MOTION_HD DcShiftCand dc_motion_pick_around_serial(const int64_t* wscores, int D, int cy, int cx) {
  const int nd = 2 * D + 1;
  DcShiftCand best = dc_motion_cand_around(wscores, D, 0, cy, cx);
  for (int i = 1; i < nd * nd; ++i) {
    const DcShiftCand c = dc_motion_cand_around(wscores, D, i, cy, cx);
    if (dc_motion_before(c, best)) best = c;
  }
  return best;
}
