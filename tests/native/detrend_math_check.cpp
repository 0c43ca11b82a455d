// Stand-alone host check of deep_calcium_amd/csrc/detrend_math.h (the scalar arithmetic of the detrended, segment-pooled
// correlations), meant to be built with -fsanitize=address,undefined and run as a program of its own
// (tests/test_detrend_api.py does that):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all detrend_math_check.cpp -o check && ./check
// The oracle is the compiler's __int128 (signed: an overflow of the oracle itself would be reported by the sanitizer).  The fold
// arithmetic is driven at the limits the header derives its magnitudes for: pixels at -32768 / 65535, L = 4096 with the longest
// last segment L_last = 8191, the largest T (2^31 - 1 for pixel pairs) and, for the footprints, the largest area and T the rules
// M * H * W <= 2^46 and T * H * W <= 2^46 allow.  Every pooled numerator must equal the oracle's (so no DcI128 intermediate
// wrapped) and stay inside the bound the header states.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../deep_calcium_amd/csrc/detrend_math.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                     \
  do {                                                       \
    if (!(cond)) {                                           \
      if (++g_fail <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
    }                                                        \
  } while (0)

typedef unsigned __int128 u128;
typedef __int128 i128;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}

static i128 wide(DcI128 a) { return (i128)(((u128)(uint64_t)a.hi << 64) | a.lo); }
static DcI128 narrow(i128 v) { DcI128 r; r.lo = (uint64_t)(u128)v; r.hi = (int64_t)(v >> 64); return r; }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static i128 iabs(i128 v) { return v < 0 ? -v : v; }

// A segment of `len` frames in which two pixels take two value pairs: (x0, y0) for k frames, (x1, y1) for the other len - k.
struct Seg { int64_t len, mult, k, x0, y0, x1, y1; };

static void seg_moments(const Seg& s, i128* ax, i128* ay, i128* gxx, i128* gxy, i128* gyy) {
  const i128 k = s.k, m = s.len - s.k;
  *ax = k * s.x0 + m * s.x1;
  *ay = k * s.y0 + m * s.y1;
  *gxx = k * s.x0 * s.x0 + m * s.x1 * s.x1;
  *gxy = k * s.x0 * s.y0 + m * s.x1 * s.y1;
  *gyy = k * s.y0 * s.y0 + m * s.y1 * s.y1;
}

int main() {
  const int64_t L = DC_DETREND_MAX_FRAMES, LAST = DC_DETREND_MAX_SEGMENT, M = L * LAST;
  CHECK(L == 4096 && LAST == 8191 && DC_DETREND_MIN_FRAMES == 2, "the limits");

  // ---- pixel with pixel at the largest T: n - 1 segments of 4096 frames and one of 8191, T <= 2^31 - 1 ---------------------------
  for (int pass = 0; pass < 4; ++pass) {
    const int64_t full = (DC_FP_MAX_FRAMES - LAST) / L, T = full * L + LAST;
    CHECK(T <= DC_FP_MAX_FRAMES && T + L > DC_FP_MAX_FRAMES, "T = %lld is not the largest", (long long)T);
    const bool uns = (pass & 1) != 0;
    const int64_t lo = uns ? 0 : -32768, hi = uns ? 65535 : 32767;
    DcI128 nxx = {0, 0}, nxy = {0, 0}, nyy = {0, 0};
    i128 wxx = 0, wxy = 0, wyy = 0;
    for (int64_t s = 0; s <= full; ++s) {
      Seg g;
      g.len = s < full ? L : LAST;
      g.mult = s < full ? LAST : L;
      CHECK(g.len * g.mult == M && dc_detrend_segment_ok(g.len, g.mult), "segment %lld", (long long)s);
      // pass 0, 1: the extremes, half and half (the largest variance); pass 2, 3: random values and splits
      g.k = pass < 2 ? g.len / 2 : (int64_t)(rng() % (uint64_t)(g.len + 1));
      g.x0 = pass < 2 ? hi : lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1));
      g.x1 = pass < 2 ? lo : lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1));
      g.y0 = pass < 2 ? ((s & 1) ? lo : hi) : lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1));
      g.y1 = pass < 2 ? ((s & 1) ? hi : lo) : lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1));
      i128 ax, ay, gxx, gxy, gyy;
      seg_moments(g, &ax, &ay, &gxx, &gxy, &gyy);
      const i128 lim63 = (i128)1 << 63;
      CHECK(gxx < lim63 && gyy < lim63 && iabs(gxy) < lim63, "a segment's g leaves int64");
      const i128 txx = (i128)g.mult * ((i128)g.len * gxx - ax * ax), txy = (i128)g.mult * ((i128)g.len * gxy - ax * ay),
                 tyy = (i128)g.mult * ((i128)g.len * gyy - ay * ay);
      const DcI128 dxx = dc_detrend_term(g.len, g.mult, (int64_t)gxx, (int64_t)ax, (int64_t)ax),
                   dxy = dc_detrend_term(g.len, g.mult, (int64_t)gxy, (int64_t)ax, (int64_t)ay),
                   dyy = dc_detrend_term(g.len, g.mult, (int64_t)gyy, (int64_t)ay, (int64_t)ay);
      CHECK(wide(dxx) == txx && wide(dxy) == txy && wide(dyy) == tyy, "term of segment %lld, pass %d", (long long)s, pass);
      CHECK(txx >= 0 && tyy >= 0 && txx <= ((i128)M * g.len << 32), "term magnitude, segment %lld", (long long)s);
      nxx = dc_i128_add(nxx, dxx); nxy = dc_i128_add(nxy, dxy); nyy = dc_i128_add(nyy, dyy);
      wxx += txx; wxy += txy; wyy += tyy;
    }
    CHECK(wide(nxx) == wxx && wide(nxy) == wxy && wide(nyy) == wyy, "pooled numerators, pass %d", pass);
    CHECK(wxx < ((i128)1 << 95) && wyy < ((i128)1 << 95) && iabs(wxy) < ((i128)1 << 95), "pooled magnitude, pass %d", pass);
    DcFpNum n = {nxx, nxy, nyy}, sw = {nyy, nxy, nxx}, dg = {nxx, nxx, nxx};
    const float r = dc_fp_corr(n);
    CHECK(r >= -1.f && r <= 1.f && bits(r) == bits(dc_fp_corr(sw)), "corr %.9g: range or symmetry, pass %d", (double)r, pass);
    CHECK(dc_fp_corr(dg) == 1.f, "diagonal, pass %d", pass);
    if (pass < 2) CHECK(wxx > ((i128)1 << 85), "pass %d does not reach the magnitudes it is meant to: %g", pass, (double)wxx);
    const double sd = sqrt(dc_detrend_var(nxx, M, T));
    const long double want = sqrtl((long double)wxx / ((long double)M * (long double)T));
    CHECK(fabsl((long double)(float)sd - want) <= want * 6.0e-8L, "std = %.9g, long double gives %.9Lg", sd, want);
  }

  // ---- one segment is today's numerators: len = T, mult = 1 ------------------------------------------------------------------------
  for (int i = 0; i < 20000; ++i) {
    const int64_t T = i % 4 == 0 ? DC_FP_MAX_FRAMES : 1 + (int64_t)(rng() % (uint64_t)DC_FP_MAX_FRAMES >> (rng() % 31));
    Seg g = {T, 1, (int64_t)(rng() % (uint64_t)(T + 1)), (int64_t)(rng() % 65536) - (i & 1 ? 0 : 32768), (int64_t)(rng() % 65536) - (i & 1 ? 0 : 32768),
             (int64_t)(rng() % 65536) - (i & 1 ? 0 : 32768), (int64_t)(rng() % 65536) - (i & 1 ? 0 : 32768)};
    i128 ax, ay, gxx, gxy, gyy;
    seg_moments(g, &ax, &ay, &gxx, &gxy, &gyy);
    const DcFpNum today = dc_pair_numerators(T, (int64_t)ax, (int64_t)ay, (int64_t)gxx, (int64_t)gxy, (int64_t)gyy);
    const DcI128 dxx = dc_detrend_term(T, 1, (int64_t)gxx, (int64_t)ax, (int64_t)ax), dxy = dc_detrend_term(T, 1, (int64_t)gxy, (int64_t)ax, (int64_t)ay),
                 dyy = dc_detrend_term(T, 1, (int64_t)gyy, (int64_t)ay, (int64_t)ay);
    CHECK(wide(dxx) == wide(today.cxx) && wide(dxy) == wide(today.cxl) && wide(dyy) == wide(today.cll), "one segment, T = %lld", (long long)T);
    CHECK(dc_detrend_segment_ok(T, 1), "one segment of %lld frames refused", (long long)T);
  }

  // ---- footprints at the largest area and T the volume rules allow --------------------------------------------------------------------
  {
    const int64_t A = DC_DETREND_MAX_VOLUME / M;                       // M * A <= 2^46 < M * (A + 1)
    const int64_t full = (DC_DETREND_MAX_VOLUME / A - LAST) / L, T = full * L + LAST;      // T * A <= 2^46
    CHECK(dc_detrend_volume_ok(L, LAST, A) && !dc_detrend_volume_ok(L, LAST, A + 1), "the largest area is %lld", (long long)A);
    CHECK((i128)T * A <= DC_DETREND_MAX_VOLUME && (i128)(T + L) * A > DC_DETREND_MAX_VOLUME, "T = %lld is not the largest", (long long)T);
    for (int pass = 0; pass < 4; ++pass) {
      const bool uns = (pass & 1) != 0;
      const int64_t lo = uns ? 0 : -32768, hi = uns ? 65535 : 32767;
      DcI128 pxx = {0, 0}, pxs = {0, 0}, pss = {0, 0};
      i128 wxx = 0, wxs = 0, wss = 0;
      for (int64_t s = 0; s <= full; ++s) {
        const int64_t len = s < full ? L : LAST, mult = s < full ? LAST : L;
        // the pixel x and the ROI's trace S (every one of its A pixels at the same extreme) over the segment: two levels
        const int64_t k = pass < 2 ? len / 2 : (int64_t)(rng() % (uint64_t)(len + 1)), m = len - k;
        const int64_t x0 = pass < 2 ? hi : lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1)), x1 = pass < 2 ? lo : lo + (int64_t)(rng() % (uint64_t)(hi - lo + 1));
        const int64_t S0 = (pass < 2 ? ((s & 1) ? lo : hi) : ((rng() & 1) ? lo : hi)) * A, S1 = (pass < 2 ? ((s & 1) ? hi : lo) : ((rng() & 1) ? lo : hi)) * A;
        const i128 a = (i128)k * x0 + (i128)m * x1, b = (i128)k * x0 * x0 + (i128)m * x1 * x1, c = (i128)k * x0 * S0 + (i128)m * x1 * S1,
                   u = (i128)k * S0 + (i128)m * S1, w = (i128)k * S0 * S0 + (i128)m * S1 * S1;
        CHECK(iabs(u) < ((i128)1 << 63) && b < ((i128)1 << 63), "u or b leaves int64");
        const i128 txx = (i128)mult * ((i128)len * b - a * a), txs = (i128)mult * ((i128)len * c - a * u), tss = (i128)mult * ((i128)len * w - u * u);
        const DcI128 dxx = dc_detrend_term(len, mult, (int64_t)b, (int64_t)a, (int64_t)a),
                     dxs = dc_detrend_term_wide(len, mult, narrow(c), (int64_t)a, (int64_t)u),
                     dss = dc_detrend_term_wide(len, mult, narrow(w), (int64_t)u, (int64_t)u);
        CHECK(wide(dxx) == txx && wide(dxs) == txs && wide(dss) == tss, "footprint term of segment %lld, pass %d", (long long)s, pass);
        pxx = dc_i128_add(pxx, dxx); pxs = dc_i128_add(pxs, dxs); pss = dc_i128_add(pss, dss);
        wxx += txx; wxs += txs; wss += tss;
      }
      CHECK(wide(pxx) == wxx && wide(pxs) == wxs && wide(pss) == wss, "pooled footprint numerators, pass %d", pass);
      CHECK(wss >= 0 && wss <= ((i128)1 << 124) && iabs(wxs) <= ((i128)1 << 110) && wxx < ((i128)1 << 95), "pooled footprint magnitudes, pass %d", pass);
      if (pass < 2) CHECK(wss > ((i128)1 << 120), "pass %d does not reach the magnitudes it is meant to: %g", pass, (double)wss);
      const DcFpNum halo = dc_detrend_fp_numerators(pxx, pxs, pss, false), in = dc_detrend_fp_numerators(pxx, pxs, pss, true);
      CHECK(wide(halo.cxx) == wxx && wide(halo.cxl) == wxs && wide(halo.cll) == wss, "halo rule, pass %d", pass);
      CHECK(wide(in.cxx) == wxx && wide(in.cxl) == wxs - wxx && wide(in.cll) == wss - 2 * wxs + wxx, "inside rule, pass %d", pass);
      CHECK(wide(in.cll) >= 0 && wide(in.cll) <= ((i128)1 << 124) && iabs(wss - 2 * wxs) < ((i128)1 << 125), "inside magnitudes, pass %d", pass);
      const float r = dc_fp_corr(halo), ri = dc_fp_corr(in);
      CHECK(r >= -1.f && r <= 1.f && ri >= -1.f && ri <= 1.f, "footprint corr %.9g / %.9g outside [-1, 1]", (double)r, (double)ri);
    }
  }

  // ---- flat series, and the acceptance of segments ----------------------------------------------------------------------------------
  {
    // constant within every segment, but at another level in each: every pooled numerator is 0 and the correlation exactly 0
    DcI128 n = {0, 0};
    const int64_t level[3] = {65535, -32768, 7};
    for (int s = 0; s < 3; ++s) n = dc_i128_add(n, dc_detrend_term(L, LAST, level[s] * level[s] * L, level[s] * L, level[s] * L));
    DcFpNum f = {n, n, n};
    CHECK(dc_i128_is_zero(n) && dc_fp_corr(f) == 0.f && !signbit(dc_fp_corr(f)), "a series constant within every segment");
    CHECK(!dc_detrend_segment_ok(0, 1) && !dc_detrend_segment_ok(1, 0) && !dc_detrend_segment_ok(-5, 3), "empty or negative");
    CHECK(dc_detrend_segment_ok(8191, 8191) && !dc_detrend_segment_ok(8192, 2) && !dc_detrend_segment_ok(2, 8192), "a segment beside others");
    CHECK(dc_detrend_segment_ok(DC_FP_MAX_FRAMES, 1) && !dc_detrend_segment_ok(DC_FP_MAX_FRAMES + 1, 1), "one segment alone");
    CHECK(dc_detrend_volume_ok(DC_FP_MAX_FRAMES, 1, 32768) && !dc_detrend_volume_ok(DC_FP_MAX_FRAMES, 1, 32769), "M = T against the area");
    CHECK(!dc_detrend_volume_ok(2, 2, ((int64_t)1 << 30) + 1) && !dc_detrend_volume_ok(2, 2, -1), "area out of range");
  }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("detrend_math_check: ok\n");
  return 0;
}
