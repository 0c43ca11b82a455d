// Stand-alone host check of the AR(2) solve of the trace dynamics, dc_dyn_ar2_solve in deep_calcium_amd/csrc/trace_dyn_math.h,
// meant to be built with -fsanitize=address,undefined and run as a program of its own (tests/test_dynamics_ar2_api.py does that):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all trace_dyn_ar2_check.cpp -o check && ./check
// Every xc is a heap buffer of exactly lags + 1 doubles, so a read past either end is reported.  The oracles are restatements:
// the same order written out once more (every bit), an exact AR(2) autocovariance (the coefficients come back), long double on
// perturbed ones within the conditioning of the 2 x 2 system, and the undefined cases.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../deep_calcium_amd/csrc/trace_dyn_math.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                     \
  do {                                                       \
    if (!(cond)) {                                           \
      if (++g_fail <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
    }                                                        \
  } while (0)

typedef long double ld;

static uint64_t rng_state = 0x2545F4914F6CDD1Dull;
static uint64_t rng() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}
static double uniform() { return (double)(rng() >> 11) * (1.0 / 9007199254740992.0); }
static uint64_t bits(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }

// xc_0 = v, xc_1 = v g1 / (1 - g2), xc_k = g1 xc_(k-1) + g2 xc_(k-2): the autocovariance of an AR(2) process without noise
static std::vector<double> ar2_autocov(double d, double r, int lags, double v) {
  const double g1 = d + r, g2 = -(d * r);
  std::vector<double> xc((size_t)lags + 1);
  xc[0] = v;
  xc[1] = v * g1 / (1.0 - g2);
  for (int k = 2; k <= lags; ++k) xc[(size_t)k] = g1 * xc[(size_t)k - 1] + g2 * xc[(size_t)k - 2];
  return xc;
}

// the header's order once more, with the rows materialised first
static void restated(const std::vector<double>& xc, int lags, double sn, long T, double* g1, double* g2) {
  std::vector<double> a((size_t)lags), b((size_t)lags), y((size_t)lags);
  const double c0 = xc[0] - sn * sn;
  for (int i = 0; i < lags; ++i) {
    a[(size_t)i] = i == 0 ? c0 : xc.at((size_t)i);
    b[(size_t)i] = i == 0 ? xc.at(1) : i == 1 ? c0 : xc.at((size_t)i - 1);
    y[(size_t)i] = xc.at((size_t)i + 1);
  }
  double Saa = 0.0, Sab = 0.0, Sbb = 0.0, Say = 0.0, Sby = 0.0;
  for (int i = 0; i < lags; ++i) Saa = Saa + a[(size_t)i] * a[(size_t)i];
  for (int i = 0; i < lags; ++i) Sab = Sab + a[(size_t)i] * b[(size_t)i];
  for (int i = 0; i < lags; ++i) Sbb = Sbb + b[(size_t)i] * b[(size_t)i];
  for (int i = 0; i < lags; ++i) Say = Say + a[(size_t)i] * y[(size_t)i];
  for (int i = 0; i < lags; ++i) Sby = Sby + b[(size_t)i] * y[(size_t)i];
  const double det = Saa * Sbb - Sab * Sab;
  *g1 = *g2 = NAN;
  if (T < lags + 2 || !(det > 0.0)) return;
  const double q1 = (Say * Sbb - Sby * Sab) / det, q2 = (Saa * Sby - Sab * Say) / det;
  if (isfinite(q1) && isfinite(q2)) { *g1 = q1; *g2 = q2; }
}

int main() {
  const double roots[][2] = {{0.75, 0.25}, {0.8824969025845955, 0.6065306597126334}, {0.99, 0.9}, {0.5, 0.01}, {0.95, 0.3}};
  for (int lags = 2; lags <= DC_DYN_MAX_LAGS; ++lags) {
    for (const auto& dr : roots) {
      const double d = dr[0], r = dr[1], g1 = d + r, g2 = -(d * r);
      // ---- an exact AR(2) autocovariance: the coefficients come back ----
      std::vector<double> xc = ar2_autocov(d, r, lags, 2.5);
      double e1 = -7.0, e2 = -7.0;
      dc_dyn_ar2_solve(xc.data(), lags, 0.0, 1000, &e1, &e2);
      CHECK(fabs(e1 - g1) < 1e-7 && fabs(e2 - g2) < 1e-7, "lags %d, roots %g %g: (%.17g, %.17g), not (%.17g, %.17g)", lags, d, r, e1, e2, g1, g2);
      // white noise of variance sn^2 adds sn^2 to xc_0 only: removed on the diagonal, the same coefficients
      const double sn = 0.7;
      xc[0] = xc[0] + sn * sn;
      dc_dyn_ar2_solve(xc.data(), lags, sn, 1000, &e1, &e2);
      CHECK(fabs(e1 - g1) < 1e-6 && fabs(e2 - g2) < 1e-6, "lags %d, roots %g %g with noise: (%.17g, %.17g)", lags, d, r, e1, e2);
      // ---- perturbed: every bit of the restatement, and long double within the conditioning ----
      for (int rep = 0; rep < 50; ++rep) {
        std::vector<double> p = ar2_autocov(d, r, lags, 0.1 + 10.0 * uniform());
        for (double& v : p) v = v * (1.0 + 0.02 * (uniform() - 0.5));
        const double s = 0.3 * uniform() * sqrt(p[0]);
        double a1, a2, b1, b2;
        dc_dyn_ar2_solve(p.data(), lags, s, 1000, &a1, &a2);
        restated(p, lags, s, 1000, &b1, &b2);
        CHECK(bits(a1) == bits(b1) && bits(a2) == bits(b2), "lags %d rep %d: (%.17g, %.17g) against the restatement (%.17g, %.17g)", lags, rep, a1, a2, b1, b2);
        ld Saa = 0, Sab = 0, Sbb = 0, Say = 0, Sby = 0;
        const ld c0 = (ld)p[0] - (ld)s * s;
        for (int i = 0; i < lags; ++i) {
          const ld a = i == 0 ? c0 : (ld)p[(size_t)i], b = i == 0 ? (ld)p[1] : i == 1 ? c0 : (ld)p[(size_t)i - 1], y = p[(size_t)i + 1];
          Saa += a * a; Sab += a * b; Sbb += b * b; Say += a * y; Sby += b * y;
        }
        const ld det = Saa * Sbb - Sab * Sab;
        if (det > 0 && !isnan(a1)) {
          const ld cond = Saa * Sbb / det, w1 = (Say * Sbb - Sby * Sab) / det, w2 = (Saa * Sby - Sab * Say) / det;
          const ld tol = 1e-13L * cond * cond * (1 + fabsl(w1) + fabsl(w2));
          CHECK(fabsl((ld)a1 - w1) <= tol && fabsl((ld)a2 - w2) <= tol, "lags %d rep %d: (%.17g, %.17g) against long double (%.17Lg, %.17Lg), cond %Lg", lags,
                rep, a1, a2, w1, w2, cond);
        }
      }
      // ---- T decides whether the estimate is defined ----
      xc = ar2_autocov(d, r, lags, 1.0);
      dc_dyn_ar2_solve(xc.data(), lags, 0.0, (long)lags + 1, &e1, &e2);
      CHECK(isnan(e1) && isnan(e2), "T = lags + 1 is defined at lags %d", lags);
      dc_dyn_ar2_solve(xc.data(), lags, 0.0, (long)lags + 2, &e1, &e2);
      CHECK(!isnan(e1) && !isnan(e2), "T = lags + 2 is undefined at lags %d", lags);
      dc_dyn_ar2_solve(xc.data(), lags, 0.0, 0, &e1, &e2);
      CHECK(isnan(e1) && isnan(e2), "T = 0 is defined at lags %d", lags);
    }
    // ---- the undefined cases: a zero system, a singular one, one that is not finite ----
    std::vector<double> zero((size_t)lags + 1, 0.0);
    double e1 = -7.0, e2 = -7.0;
    dc_dyn_ar2_solve(zero.data(), lags, 0.0, 1000, &e1, &e2);
    CHECK(isnan(e1) && isnan(e2), "an all-zero xc is defined at lags %d", lags);
    std::vector<double> flat((size_t)lags + 1, 1.0);                  // a == b in every row: det == 0 exactly
    dc_dyn_ar2_solve(flat.data(), lags, 0.0, 1000, &e1, &e2);
    CHECK(isnan(e1) && isnan(e2), "a singular system is defined at lags %d: %g %g", lags, e1, e2);
    std::vector<double> huge((size_t)lags + 1, 1e200);
    huge[0] = 2e200;
    dc_dyn_ar2_solve(huge.data(), lags, 0.0, 1000, &e1, &e2);
    CHECK(isnan(e1) && isnan(e2), "an overflowing system is defined at lags %d: %g %g", lags, e1, e2);
    std::vector<double> nan((size_t)lags + 1, 1.0);
    nan[(size_t)lags] = NAN;
    dc_dyn_ar2_solve(nan.data(), lags, 0.0, 1000, &e1, &e2);
    CHECK(isnan(e1) && isnan(e2), "a NaN covariance gives a number at lags %d", lags);
    // the noise above the variance: c0 < 0 is legal, the result is whatever the arithmetic gives, and it matches the restatement
    std::vector<double> xc = ar2_autocov(0.9, 0.5, lags, 1.0);
    double b1, b2;
    dc_dyn_ar2_solve(xc.data(), lags, 3.0, 1000, &e1, &e2);
    restated(xc, lags, 3.0, 1000, &b1, &b2);
    CHECK(bits(e1) == bits(b1) && bits(e2) == bits(b2), "c0 < 0 at lags %d", lags);
  }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("trace_dyn_ar2_check: ok\n");
  return 0;
}
