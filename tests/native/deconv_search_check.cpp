// Stand-alone host check of the noise-constrained search, deep_calcium_amd/csrc/deconv_search_math.h (dc_search_step and the host
// search built on it), meant to be built with -fsanitize=address,undefined and run as a program of its own
// (tests/test_deconv_search_api.py does that):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all deconv_search_check.cpp -o check && ./check
// (1) The step against a model residual r(p) = p: the bracket follows the rule round by round and its width is the promised
// 2^max(e-2, 0) sigma / 2^(N-e), to the rounding of the midpoints (half an ulp of hi a round).  (2) The host search over ragged
// T, 1 .. 700 frames, both parameters: the buffers are exactly T long, so a read or write past a trace is the sanitizer's; RSS(p*)
// recomputed is the one reported and within the target, the status is the one the residuals imply, and the fold agrees with a
// long double sum.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../deep_calcium_amd/csrc/deconv_search_math.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                     \
  do {                                                       \
    if (!(cond)) {                                           \
      if (++g_fail <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
    }                                                        \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}
static double uniform() { return (double)(rng() >> 11) * (1.0 / 9007199254740992.0); }
static double normal() {                                     // sum of 12 uniforms: good enough for noise
  double s = -6.0;
  for (int i = 0; i < 12; ++i) s += uniform();
  return s;
}

// r(p) = p and target = sigma * sigma * T chosen freely: the search is a bisection for the target itself
static void model_search(double sigma, long T, int rounds) {
  DcSearch s = dc_search_begin(sigma, T);
  CHECK(s.target == (sigma * sigma) * (double)T && s.phase == DC_SEARCH_START, "begin");
  double p = dc_search_step(s, 0.0, 0.0);                    // round 0: r0 = 0
  if (!(0.0 < s.target)) {
    CHECK(s.phase == DC_SEARCH_DONE && p == 0.0 && dc_search_status(s) == 1, "sigma = %g: not finished", sigma);
    for (int i = 0; i < rounds; ++i) p = dc_search_step(s, p, 0.0);
    CHECK(s.lo == 0.0 && s.rss_lo == 0.0 && p == 0.0 && dc_search_status(s) == 1, "sigma = %g: a finished search moved", sigma);
    return;
  }
  CHECK(p == sigma && s.phase == DC_SEARCH_EXPAND, "round 1 does not try sigma");
  int e = 0;
  for (int i = 1; i <= rounds; ++i) {
    const bool expanding = s.phase == DC_SEARCH_EXPAND;
    CHECK(p == (expanding ? s.hi : 0.5 * (s.lo + s.hi)), "round %d tries %g", i, p);
    if (expanding) ++e;
    p = dc_search_step(s, p, p);
    CHECK(s.rss_lo <= s.target && s.lo == s.rss_lo, "round %d: lo = %g is over the target %g", i, s.lo, s.target);
    if (s.phase == DC_SEARCH_BISECT) CHECK(s.hi > s.target, "round %d: hi = %g is not over the target %g", i, s.hi, s.target);
  }
  if (dc_search_status(s) == 0)
    CHECK(fabs(s.hi - s.lo - ldexp(sigma, (e >= 2 ? e - 2 : 0) - (rounds - e))) <= rounds * 0x1p-52 * s.hi, "sigma %g, T %ld, %d rounds, %d expanding: hi - lo = %g", sigma, T, rounds, e, s.hi - s.lo);
  else
    CHECK(dc_search_status(s) == 2 && e == rounds && s.lo == ldexp(sigma, rounds - 1) && s.hi == ldexp(sigma, rounds), "never bracketed: lo = %g", s.lo);
}

template <typename In>
static void run_trace(const std::vector<In>& y, double g, int which, double sigma, double other, int rounds, int expect, const char* what) {
  const long T = (long)y.size();
  std::vector<double> G((size_t)T + 1);
  G[0] = 1.0;
  for (long l = 1; l <= T; ++l) G[(size_t)l] = G[(size_t)l - 1] * g;
  std::vector<DcPool> pool((size_t)T);
  std::vector<double> c((size_t)T);
  double param = -1.0, rss = -1.0;
  int32_t status = -1;
  dc_search_host(y.data(), T, DcAr1{g, G.data()}, which, sigma, other, rounds, pool, c.data(), &param, &rss, &status);
  const double target = dc_search_target(sigma, T);
  auto residual = [&](double p) {
    const int32_t n = which == DC_SEARCH_LAM ? dc_deconv_forward_host(y.data(), T, g, G.data(), p, other, pool)
                                             : dc_deconv_forward_host(y.data(), T, g, G.data(), other, p, pool);
    return dc_rss_host(y.data(), T, DcAr1{g, G.data()}, pool, n, c.data());
  };
  const double r0 = residual(0.0), again = residual(param);
  CHECK(status >= 0 && status <= 2 && param >= 0.0 && again == rss, "%s: status %d, p* = %g, RSS %g reported as %g", what, status, param, again, rss);
  CHECK((status == 1) == !(r0 < target), "%s: status %d with RSS(0) = %g, target %g", what, status, r0, target);
  if (status == 1) CHECK(param == 0.0, "%s: status 1 with p* = %g", what, param);
  else CHECK(rss <= target, "%s: RSS(p*) = %g is over the target %g", what, rss, target);
  if (status == 2) CHECK(param == ldexp(sigma, rounds - 1), "%s: never bracketed but p* = %g", what, param);
  if (expect >= 0) CHECK(status == expect, "%s: status %d, not %d", what, status, expect);
  // the fold against a long double sum of the same terms
  long double wide = 0.0L;
  for (long t = 0; t < T; ++t) wide += (long double)dc_search_term((double)y[(size_t)t], c[(size_t)t]);
  CHECK(fabsl((long double)again - wide) <= 1e-12L * (wide > 1.0L ? wide : 1.0L), "%s: fold %g against %Lg", what, again, wide);
}

int main() {
  CHECK(dc_search_term(3.0, 1.0) == 4.0 && dc_search_term(1.0, 3.0) == 4.0 && dc_search_target(0.5, 8) == 2.0, "term / target");
  const double sigmas[] = {0.0, 1e-200, 0.1, 0.3, 1.0, 37.5, 0x1p499};
  for (double sigma : sigmas)
    for (long T : {1L, 2L, 600L, 16777216L})
      for (int rounds : {1, 2, 5, 24, 64}) model_search(sigma, T, rounds);

  const double gs[] = {exp(-1.0 / 2), exp(-1.0 / 8), exp(-1.0 / 30)};
  for (long T : {1L, 2L, 3L, 255L, 256L, 257L, 700L}) {
    std::vector<double> zero((size_t)T, 0.0);
    for (int rounds : {1, 5, 24, 64}) {
      run_trace(zero, gs[1], DC_SEARCH_SMIN, 1.0, 0.0, rounds, 2, "zero, smin");
      run_trace(zero, gs[1], DC_SEARCH_LAM, 1.0, 0.0, rounds, 2, "zero, lam");
    }
    run_trace(zero, gs[1], DC_SEARCH_SMIN, 0.0, 0.0, 24, 1, "zero, sigma 0");
  }
  for (int i = 0; i < 240; ++i) {
    const long T = 1 + (long)(rng() % 700);
    const double g = gs[i % 3], noise = 0.05 + 0.5 * uniform();
    std::vector<double> y((size_t)T);
    std::vector<float> yf((size_t)T);
    double c = 0.0;
    for (long t = 0; t < T; ++t) {
      c = c * g + (uniform() < 0.05 ? 1.0 : 0.0);
      y[(size_t)t] = c + noise * normal();
      yf[(size_t)t] = (float)y[(size_t)t];
    }
    const int which = i & 1, rounds = 1 + (int)(rng() % 30);
    const double other = (i % 4) >= 2 ? 0.1 * uniform() : 0.0;
    run_trace(y, g, which, noise, other, rounds, -1, "random");
    run_trace(yf, g, which, 0.5 * noise, other, rounds, -1, "random, float");
    run_trace(y, g, which, 0.0, other, rounds, 1, "random, sigma 0");
  }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("deconv_search_check: ok\n");
  return 0;
}
