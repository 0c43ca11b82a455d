// Stand-alone host check of deep_calcium_amd/csrc/pair_math.h (the scalar arithmetic of the ROI pixel-pair correlation), meant to
// be built with -fsanitize=address,undefined and run as a program of its own (tests/test_roi_pairs_api.py does that):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all pair_math_check.cpp -o check && ./check
// The oracle is the compiler's __int128 (signed: an overflow of the oracle itself would be reported by the sanitizer), at the
// limit T = 2^31 - 1 with pixels at -32768 / 65535, plus the properties the header promises of the correlation: the same bits
// for (i, j) and (j, i), a diagonal of exactly 1, exactly 0 for a constant pixel, exactly +-1 for equal and mirrored series,
// and never outside [-1, 1].
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../deep_calcium_amd/csrc/pair_math.h"

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
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// two series of n distinct (x, y) pairs, pair k held for reps[k] frames
struct Pair {
  int n;
  int64_t x[6], y[6], reps[6];
  int64_t T;
};

static void moments(const Pair& s, i128* ax, i128* ay, i128* gxx, i128* gxy, i128* gyy) {
  *ax = *ay = *gxx = *gxy = *gyy = 0;
  for (int k = 0; k < s.n; ++k) {
    *ax += (i128)s.x[k] * s.reps[k];
    *ay += (i128)s.y[k] * s.reps[k];
    *gxx += (i128)s.x[k] * s.x[k] * s.reps[k];
    *gxy += (i128)s.x[k] * s.y[k] * s.reps[k];
    *gyy += (i128)s.y[k] * s.y[k] * s.reps[k];
  }
}

static float corr_of(const Pair& s, bool swapped = false, DcFpNum* num_out = 0) {
  i128 ax, ay, gxx, gxy, gyy;
  moments(s, &ax, &ay, &gxx, &gxy, &gyy);
  const DcFpNum n = swapped ? dc_pair_numerators(s.T, (int64_t)ay, (int64_t)ax, (int64_t)gyy, (int64_t)gxy, (int64_t)gxx)
                            : dc_pair_numerators(s.T, (int64_t)ax, (int64_t)ay, (int64_t)gxx, (int64_t)gxy, (int64_t)gyy);
  if (num_out) *num_out = n;
  return dc_fp_corr(n);
}

int main() {
  // ---- the numerators at the limits, symmetry, range -----------------------------------------------------------------------------
  for (int i = 0; i < 20000; ++i) {
    const int64_t T = i % 4 == 0 ? DC_FP_MAX_FRAMES : 1 + (int64_t)(rng() % (uint64_t)DC_FP_MAX_FRAMES >> (rng() % 31));
    const bool uns = (rng() & 1) != 0, extreme = i % 3 == 0;
    const int64_t xmin = uns ? 0 : -32768, xmax = uns ? 65535 : 32767;
    Pair s;
    s.n = T < 6 ? (int)T : 6;
    s.T = T;
    for (int k = 0; k < s.n; ++k) {
      s.reps[k] = T / s.n + (k == 0 ? T % s.n : 0);
      s.x[k] = extreme ? ((rng() & 1) ? xmax : xmin) : xmin + (int64_t)(rng() % (uint64_t)(xmax - xmin + 1));
      s.y[k] = extreme ? ((rng() & 1) ? xmax : xmin) : xmin + (int64_t)(rng() % (uint64_t)(xmax - xmin + 1));
    }
    i128 ax, ay, gxx, gxy, gyy;
    moments(s, &ax, &ay, &gxx, &gxy, &gyy);
    const i128 lim = (i128)1 << 63;
    CHECK(gxx < lim && gyy < lim && gxy < lim && gxy > -lim, "g leaves int64, T=%lld", (long long)T);
    const i128 cxx = (i128)T * gxx - ax * ax, cxy = (i128)T * gxy - ax * ay, cyy = (i128)T * gyy - ay * ay;
    DcFpNum n;
    const float r = corr_of(s, false, &n);
    CHECK(wide(n.cxx) == cxx && wide(n.cxl) == cxy && wide(n.cll) == cyy, "numerators T=%lld", (long long)T);
    CHECK(cxx >= 0 && cyy >= 0 && cxx < ((i128)1 << 95) && cyy < ((i128)1 << 95), "magnitudes T=%lld", (long long)T);
    CHECK(r >= -1.f && r <= 1.f, "corr = %.9g outside [-1, 1]", (double)r);
    CHECK(bits(r) == bits(corr_of(s, true)), "corr_ij and corr_ji differ, T=%lld", (long long)T);
    if (cxx > 0 && cyy > 0) {
      const long double want = (long double)cxy / (sqrtl((long double)cxx) * sqrtl((long double)cyy));
      CHECK(fabsl((long double)r - want) <= 6.1e-8L, "corr = %.9g, long double gives %.9Lg", (double)r, want);      // one float32 ulp below 1
    } else {
      CHECK(r == 0.f && !signbit(r), "corr of a flat series = %.9g", (double)r);
    }
    // the diagonal: a pixel with itself
    Pair d = s;
    for (int k = 0; k < s.n; ++k) d.y[k] = d.x[k];
    CHECK(corr_of(d) == (cxx > 0 ? 1.f : 0.f), "diagonal = %.9g, T=%lld", (double)corr_of(d), (long long)T);
  }

  // ---- the edge cases ------------------------------------------------------------------------------------------------------------
  {
    Pair c = {3, {5, 5, 5}, {100, -7, 30}, {4, 4, 4}, 12};                          // a pixel constant in time: row, column, diagonal
    CHECK(corr_of(c) == 0.f && corr_of(c, true) == 0.f, "constant pixel");
    Pair cc = {3, {5, 5, 5}, {5, 5, 5}, {4, 4, 4}, 12};
    CHECK(corr_of(cc) == 0.f && !signbit(corr_of(cc)), "constant pixel, diagonal");
    Pair one = {1, {65535}, {-32768}, {1}, 1};                                      // T == 1
    CHECK(corr_of(one) == 0.f, "T == 1");
    Pair top = {2, {65535, 0}, {65535, 0}, {DC_FP_MAX_FRAMES - 1, 1}, DC_FP_MAX_FRAMES};      // g = 65535^2 (2^31 - 2) < 2^63
    CHECK(corr_of(top) == 1.f, "the largest g: %.9g", (double)corr_of(top));
    for (int i = 0; i < 2000; ++i) {                                                // +-1 for every such pair, not just one
      Pair p;
      p.n = 6; p.T = 0;
      for (int k = 0; k < 6; ++k) {
        p.x[k] = (int64_t)(rng() % 65536) - 32768;
        p.reps[k] = 1 + (int64_t)(rng() % 1000);
        p.y[k] = p.x[k];
        p.T += p.reps[k];
      }
      if (p.x[0] == p.x[1]) continue;
      CHECK(corr_of(p) == 1.f, "equal series %d", i);
      for (int k = 0; k < 6; ++k) p.y[k] = 12345 - p.x[k];
      CHECK(corr_of(p) == -1.f && corr_of(p, true) == -1.f, "mirrored series %d", i);
    }
  }

  // ---- the bookkeeping -------------------------------------------------------------------------------------------------------------
  {
    const int64_t ks[] = {1, 63, 64, 65, 128, 129, 130, 1024}, want[] = {1, 1, 1, 3, 3, 6, 6, 136};
    for (int i = 0; i < 8; ++i) CHECK(dc_pair_tiles_of(ks[i], 64) == want[i], "tiles of %lld", (long long)ks[i]);
    CHECK(dc_pair_roi_ok(0, 1024, 0, 1024, 1024 * 1024, 1024), "the largest ROI alone");
    CHECK(!dc_pair_roi_ok(0, 1025, 0, 2000, 1L << 27, 1024), "k over the limit");
    CHECK(!dc_pair_roi_ok(0, 10, 1, 10, 100, 1024) && dc_pair_roi_ok(0, 10, 0, 10, 100, 1024), "a square that leaves the state");
    CHECK(!dc_pair_roi_ok(-1, 10, 0, 10, 1000, 1024) && !dc_pair_roi_ok(5, 11, 0, 10, 1000, 1024) && !dc_pair_roi_ok(5, 5, 0, 10, 1000, 1024) &&
          !dc_pair_roi_ok(6, 5, 0, 10, 1000, 1024), "pixels outside the state, empty, reversed");
    CHECK(!dc_pair_roi_ok(0, 10, -1, 10, 1000, 1024) && !dc_pair_roi_ok(0, 10, INT64_MAX, 10, 1000, 1024), "goff negative or huge");
    CHECK(!dc_pair_roi_ok(INT32_MIN, INT32_MAX, 0, 10, 1000, 1024), "int32 extremes");
  }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("pair_math_check: ok\n");
  return 0;
}
