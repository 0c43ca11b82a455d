// Stand-alone host check of deep_calcium_amd/csrc/footprint_math.h (the scalar arithmetic of the ROI footprint maps), meant to be
// built with -fsanitize=address,undefined and run as a program of its own (tests/test_footprints_api.py does that):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all footprint_math_check.cpp -o check && ./check
// The oracle is the compiler's __int128 (signed: an overflow of the oracle itself would be reported by the sanitizer, so a pass
// also shows that every intermediate stays inside 127 bits), at the limits T * H * W = 2^46 and T = 2^31 - 1 with pixels at
// -32768 / 65535 and |S| up to 2^46, plus the edge cases of the correlation.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../deep_calcium_amd/csrc/footprint_math.h"

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
static DcI128 narrow(i128 v) {
  DcI128 a;
  a.lo = (uint64_t)(u128)v;
  a.hi = (int64_t)(uint64_t)((u128)v >> 64);
  return a;
}

// A series of n distinct (x, rest) pairs, pair k held for reps[k] frames; S = rest (+ x when the pixel is inside the ROI).
struct Series {
  int n;
  int64_t x[6], S[6], reps[6];
  int64_t T;
};

static void moments(const Series& s, i128* a, i128* b, i128* c, i128* u, i128* w) {
  *a = *b = *c = *u = *w = 0;
  for (int k = 0; k < s.n; ++k) {
    *a += (i128)s.x[k] * s.reps[k];
    *b += (i128)s.x[k] * s.x[k] * s.reps[k];
    *c += (i128)s.x[k] * s.S[k] * s.reps[k];
    *u += (i128)s.S[k] * s.reps[k];
    *w += (i128)s.S[k] * s.S[k] * s.reps[k];
  }
}

static float corr_of(const Series& s, bool inside, DcFpNum* num_out = 0) {
  i128 a, b, c, u, w;
  moments(s, &a, &b, &c, &u, &w);
  const DcFpNum n = dc_fp_numerators(s.T, (int64_t)a, (int64_t)b, narrow(c), (int64_t)u, narrow(w), inside);
  if (num_out) *num_out = n;
  return dc_fp_corr(n);
}

int main() {
  // ---- the split and the fold: every int64 S, runs of the kernel's length at the extremes -------------------------------------
  const int64_t e64[] = {0, 1, -1, INT64_MAX, INT64_MIN, 0xffffffffll, 0x100000000ll, -0x100000000ll, -0xffffffffll, 1ll << 46, -(1ll << 46),
                         (1ll << 46) - 1, 1 - (1ll << 46), 2147483647ll, -2147483648ll};
  const int ne = (int)(sizeof(e64) / sizeof(e64[0]));
  for (int i = 0; i < ne + 2000; ++i) {
    const int64_t S = i < ne ? e64[i] : (int64_t)(rng() >> (rng() % 64)) * ((rng() & 1) ? 1 : -1);
    uint32_t lo;
    int32_t hi;
    dc_fp_split(S, &lo, &hi);
    CHECK((i128)hi * ((i128)1 << 32) + lo == (i128)S, "split %lld", (long long)S);
    const int64_t xs[] = {-32768, 65535, 0, 1, -1, 32767};
    for (int64_t x : xs) {
      const int run = 512;                                // the kernel's kStage
      int64_t alo = 0, ahi = 0;
      for (int k = 0; k < run; ++k) { alo += x * (int64_t)lo; ahi += x * (int64_t)hi; }       // int64 overflow here: the sanitizer stops
      const i128 start = -((i128)7 << 70);
      DcI128 c = narrow(start);
      c = dc_fp_fold(c, alo, ahi);
      CHECK(wide(c) == start + (i128)run * x * S, "fold x=%lld S=%lld", (long long)x, (long long)S);
    }
  }

  // ---- the numerators at the limits -----------------------------------------------------------------------------------------------
  for (int i = 0; i < 20000; ++i) {
    int64_t hw, T;
    if (i % 5 == 0) { hw = 1ll << 30; T = 1ll << 16; }                   // |S| reaches 2^46
    else if (i % 5 == 1) { hw = 1ll << 15; T = DC_FP_MAX_FRAMES; }       // the longest recording
    else {
      hw = 1 + (int64_t)(rng() % (1ull << (rng() % 31)));
      int64_t tmax = (1ll << 46) / hw;
      if (tmax > DC_FP_MAX_FRAMES) tmax = DC_FP_MAX_FRAMES;
      T = (i & 1) ? tmax : 1 + (int64_t)(rng() % (uint64_t)tmax);
    }
    const bool uns = (rng() & 1) != 0, inside = (rng() & 2) != 0, extreme = i % 3 == 0;
    const int64_t xmin = uns ? 0 : -32768, xmax = uns ? 65535 : 32767;
    const int64_t A = inside ? hw - 1 : hw;                              // the other pixels of the ROI
    Series s;
    s.n = T < 6 ? (int)T : 6;
    s.T = T;
    for (int k = 0; k < s.n; ++k) {
      s.reps[k] = T / s.n + (k == 0 ? T % s.n : 0);
      s.x[k] = extreme ? ((rng() & 1) ? xmax : xmin) : xmin + (int64_t)(rng() % (uint64_t)(xmax - xmin + 1));
      int64_t rest = extreme ? ((rng() & 1) ? xmax * A : xmin * A) : (A == 0 ? 0 : xmin * A + (int64_t)(rng() % (uint64_t)((xmax - xmin) * A + 1)));
      s.S[k] = rest + (inside ? s.x[k] : 0);
    }
    i128 a, b, c, u, w;
    moments(s, &a, &b, &c, &u, &w);
    CHECK(b < ((i128)1 << 63) && u < ((i128)1 << 63) && u > -((i128)1 << 63), "b or u leaves int64, T=%lld hw=%lld", (long long)T, (long long)hw);
    const i128 cxx = (i128)T * b - a * a, cxs = (i128)T * c - a * u, css = (i128)T * w - u * u;
    const i128 cxl = inside ? cxs - cxx : cxs, cll = inside ? css - 2 * cxs + cxx : css;
    DcFpNum n;
    const float r = corr_of(s, inside, &n);
    CHECK(wide(n.cxx) == cxx && wide(n.cxl) == cxl && wide(n.cll) == cll, "numerators T=%lld hw=%lld inside=%d", (long long)T, (long long)hw,
          (int)inside);
    CHECK(cxx >= 0 && cll >= 0 && cll <= ((i128)1 << 124) && cxx < ((i128)1 << 94), "magnitudes T=%lld hw=%lld", (long long)T, (long long)hw);
    CHECK(r >= -1.f && r <= 1.f, "corr = %.9g outside [-1, 1]", (double)r);
    if (cxx > 0 && cll > 0) {
      const long double want = (long double)cxl / (sqrtl((long double)cxx) * sqrtl((long double)cll));
      CHECK(fabsl((long double)r - want) <= 6.1e-8L, "corr = %.9g, long double gives %.9Lg", (double)r, want);      // one float32 ulp below 1
    } else {
      CHECK(r == 0.f && !signbit(r), "corr of a flat series = %.9g", (double)r);
    }
  }

  // ---- the edge cases of the correlation ---------------------------------------------------------------------------------------
  {
    Series s = {3, {5, 5, 5}, {100, -7, 30}, {4, 4, 4}, 12};                        // a pixel constant in time
    CHECK(corr_of(s, false) == 0.f && corr_of(s, true) == 0.f, "constant pixel");
    Series t = {3, {5, -9, 300}, {77, 77, 77}, {4, 4, 4}, 12};                       // a trace constant in time
    CHECK(corr_of(t, false) == 0.f, "constant trace");
    Series one = {1, {65535}, {1ll << 46}, {1}, 1};                                  // T == 1
    CHECK(corr_of(one, false) == 0.f && corr_of(one, true) == 0.f, "T == 1");
    Series own = {3, {5, -9, 300}, {5, -9, 300}, {4, 5, 3}, 12};                     // the pixel of a one-pixel ROI: S - x == 0
    CHECK(corr_of(own, true) == 0.f, "one-pixel ROI");
    CHECK(corr_of(own, false) == 1.f, "a halo pixel equal to the trace: %.9g", (double)corr_of(own, false));
    Series mir = {3, {5, -9, 300}, {1000 - 5, 1000 + 9, 1000 - 300}, {4, 5, 3}, 12}; // the trace mirrored about a constant
    CHECK(corr_of(mir, false) == -1.f, "a halo pixel mirrored: %.9g", (double)corr_of(mir, false));
    for (int i = 0; i < 2000; ++i) {                                                 // +-1 for every such series, not just one
      Series p;
      p.n = 6; p.T = 0;
      for (int k = 0; k < 6; ++k) {
        p.x[k] = (int64_t)(rng() % 65536) - 32768;
        p.reps[k] = 1 + (int64_t)(rng() % 1000);
        p.S[k] = p.x[k];
        p.T += p.reps[k];
      }
      if (p.x[0] == p.x[1]) continue;
      CHECK(corr_of(p, false) == 1.f, "equal series %d", i);
      for (int k = 0; k < 6; ++k) p.S[k] = 12345 - p.x[k];
      CHECK(corr_of(p, false) == -1.f, "mirrored series %d", i);
    }
  }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("footprint_math_check: ok\n");
  return 0;
}
