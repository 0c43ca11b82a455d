// Stand-alone host check of the baseline in the AR(1) deconvolution, deep_calcium_amd/csrc/deconv_base_math.h (the gain term, the
// clamped Newton step, the joint search's step and the host fit and search built on them), meant to be built with
// -fsanitize=address,undefined and run as a program of its own (tests/test_deconv_base_api.py does that):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all deconv_base_check.cpp -o check && ./check
// (1) The gain term against the sums it is the closed form of, and the step's clamp.  (2) The joint step against a model residual
// r(p) = p: the bracket moves as the plain search's does, b_lo is the baseline lo was evaluated with, a finished search keeps b_0.
// (3) b = 0 gives the pools of deconv_math.h's forward pass in every bit.  (4) The host fit and the host search over ragged T,
// 1 .. 700 frames, both parameters: the buffers are exactly T long, so a read or write past a trace is the sanitizer's;
// RSS(p*, b*) recomputed is the one reported and within the target; on a long noisy trace with an offset the fitted baseline
// leaves a mean residual far below the offset.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../deep_calcium_amd/csrc/deconv_base_math.h"

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

static std::vector<double> table(double g, long T) {
  std::vector<double> G((size_t)T + 1);
  G[0] = 1.0;
  for (long l = 1; l <= T; ++l) G[(size_t)l] = G[(size_t)l - 1] * g;
  return G;
}

static void gain_and_step() {
  const double gs[] = {exp(-1.0 / 2), exp(-1.0 / 8), exp(-1.0 / 30)};
  for (double g : gs) {
    const std::vector<double> G = table(g, 400);
    long double s1 = 0.0L, s2 = 0.0L;
    for (long l = 1; l <= 400; ++l) {
      s1 += (long double)G[(size_t)l - 1];
      s2 += (long double)G[(size_t)l - 1] * (long double)G[(size_t)l - 1];
      const double a = dc_base_gain(g, G[(size_t)l]);
      const long double want = s1 * s1 / s2;
      CHECK(fabsl((long double)a - want) <= 1e-9L * want, "g %g, l %ld: gain %g against %Lg", g, l, a, want);
      CHECK(a >= 1.0 - 1e-12 && a <= (double)l * (1.0 + 1e-12), "g %g, l %ld: gain %g outside [1, l]", g, l, a);
    }
    CHECK(dc_base_gain_at(1.0, 5, 5, g, G[3]) == dc_base_gain(g, G[3]) && dc_base_gain_at(1.0, 6, 5, g, G[3]) == 0.0 &&
              dc_base_gain_at(0.0, 5, 5, g, G[3]) == 0.0 && dc_base_gain_at(-1.0, 5, 5, g, G[3]) == 0.0 && !signbit(dc_base_gain_at(-1.0, 5, 5, g, G[3])),
          "gain_at");
  }
  CHECK(dc_base_step(1.0, 8.0, 0.0, 16) == 1.5, "step, den = 1");
  CHECK(dc_base_step(1.0, 8.0, 8.0, 16) == 2.0, "step, den = 0.5");
  CHECK(dc_base_step(1.0, 8.0, 12.0, 16) == 3.0 && dc_base_step(1.0, 8.0, 16.0, 16) == 3.0 && dc_base_step(1.0, 8.0, 40.0, 16) == 3.0, "step: the clamp at 0.25");
  CHECK(dc_base_step(1.0, 8.0, NAN, 16) == 3.0, "step: a NaN gain is clamped");
  CHECK(dc_base_data(-0.0, 0.0) == 0.0 && signbit(dc_base_data(-0.0, 0.0)) && dc_base_resid(3.0, 1.0, 0.5) == 1.5, "data / resid");
}

// r(p) = p: the joint step is the plain step, and b_lo follows lo
static void model_search(double sigma, long T, int rounds) {
  DcBaseSearch q = dc_base_search_begin(sigma, T, 0.25);
  DcSearch s = dc_search_begin(sigma, T);
  CHECK(q.b == 0.25 && q.b_lo == 0.25 && q.s.phase == DC_SEARCH_START && q.s.target == s.target, "begin");
  double p = dc_base_search_step(q, 0.0, 0.0), p2 = dc_search_step(s, 0.0, 0.0);
  CHECK(p == p2 && q.b_lo == 0.25, "round 0");
  double b_of_lo = 0.25;
  for (int i = 1; i <= rounds; ++i) {
    const double b = dc_base_search_newton(q, (double)i, 0.0, T);       // b moves by i / T a round, unless the search is over
    if (q.s.phase == DC_SEARCH_DONE) CHECK(b == 0.25 && q.b == 0.25, "a finished search moved its baseline");
    else CHECK(b == q.b, "newton");
    const double lo_before = q.s.lo;
    const bool took = q.s.phase != DC_SEARCH_DONE && p <= q.s.target;
    p = dc_base_search_step(q, p, p);
    p2 = dc_search_step(s, p2, p2);
    if (took) b_of_lo = b;
    else CHECK(q.s.lo == lo_before, "lo moved without r <= target");
    CHECK(p == p2 && q.s.lo == s.lo && q.s.hi == s.hi && q.s.rss_lo == s.rss_lo && q.s.phase == s.phase, "round %d: not the plain step", i);
    CHECK(q.b_lo == b_of_lo, "round %d: b_lo = %g, lo was evaluated with %g", i, q.b_lo, b_of_lo);
  }
}

template <typename In>
static void run_trace(const std::vector<In>& y, double g, int which, double sigma, double other, double b0, int rounds, const char* what) {
  const long T = (long)y.size();
  const std::vector<double> G = table(g, T);
  std::vector<DcPool> pool((size_t)T), pool0((size_t)T);
  std::vector<double> c((size_t)T), a((size_t)T);
  // b = 0: the pools of the forward pass without a baseline
  const int32_t n0 = dc_deconv_forward_host(y.data(), T, g, G.data(), other, 0.5 * other, pool0);
  const int32_t n1 = dc_base_forward_host(y.data(), T, g, G.data(), other, 0.5 * other, 0.0, pool);
  CHECK(n0 == n1 && memcmp(pool.data(), pool0.data(), (size_t)n0 * sizeof(DcPool)) == 0, "%s: b = 0 changes the pools", what);
  // the search
  double param = -1.0, base = -1.0, rss = -1.0;
  int32_t status = -1;
  dc_base_search_host(y.data(), T, g, G.data(), which, sigma, other, b0, rounds, pool, c.data(), a.data(), &param, &base, &rss, &status);
  const double target = dc_search_target(sigma, T);
  auto sums = [&](double p, double b) {
    const int32_t n = which == DC_SEARCH_LAM ? dc_base_forward_host(y.data(), T, g, G.data(), p, other, b, pool)
                                             : dc_base_forward_host(y.data(), T, g, G.data(), other, p, b, pool);
    return dc_base_sums_host(y.data(), T, G.data(), b, pool, n, c.data(), a.data());
  };
  const double r0 = sums(0.0, b0).rss;
  const DcBaseSums again = sums(param, base);
  CHECK(status >= 0 && status <= 2 && param >= 0.0 && again.rss == rss, "%s: status %d, p* = %g, RSS %g reported as %g", what, status, param, again.rss, rss);
  CHECK((status == 1) == !(r0 < target), "%s: status %d with RSS(0, b0) = %g, target %g", what, status, r0, target);
  if (status == 1) CHECK(param == 0.0 && base == b0, "%s: status 1 with p* = %g, b* = %g", what, param, base);
  else CHECK(rss <= target, "%s: RSS(p*, b*) = %g is over the target %g", what, rss, target);
  CHECK(again.A >= 0.0 && again.A <= (double)T * (1.0 + 1e-12), "%s: A = %g outside [0, T]", what, again.A);
  long double wide = 0.0L;
  for (long t = 0; t < T; ++t) wide += (long double)dc_base_resid((double)y[(size_t)t], base, c[(size_t)t]);
  CHECK(fabsl((long double)again.S - wide) <= 1e-11L * (1.0L + fabsl(wide)) + 1e-13L * T, "%s: S %g against %Lg", what, again.S, wide);
  // the fit
  const double b = dc_base_fit_host(y.data(), T, g, G.data(), which == DC_SEARCH_LAM ? 0.1 : other, which == DC_SEARCH_LAM ? other : 0.3, b0, rounds, pool,
                                    c.data(), a.data());
  CHECK(b - b == 0.0, "%s: the fit gave %g", what, b);
}

int main() {
  gain_and_step();
  const double sigmas[] = {0.0, 1e-200, 0.1, 0.3, 1.0, 37.5, 0x1p499};
  for (double sigma : sigmas)
    for (long T : {1L, 2L, 600L, 16777216L})
      for (int rounds : {1, 2, 5, 24, 64}) model_search(sigma, T, rounds);

  const double gs[] = {exp(-1.0 / 2), exp(-1.0 / 8), exp(-1.0 / 30)};
  for (long T : {1L, 2L, 3L, 255L, 256L, 257L, 700L}) {
    std::vector<double> flat((size_t)T, 0.75);
    for (int rounds : {1, 5, 24}) {
      run_trace(flat, gs[1], DC_SEARCH_SMIN, 1.0, 0.0, 0.0, rounds, "constant, smin");
      run_trace(flat, gs[1], DC_SEARCH_LAM, 1.0, 0.0, 0.5, rounds, "constant, lam");
    }
    run_trace(flat, gs[1], DC_SEARCH_SMIN, 0.0, 0.0, 0.0, 24, "constant, sigma 0");
  }
  for (int i = 0; i < 160; ++i) {
    const long T = 1 + (long)(rng() % 700);
    const double g = gs[i % 3], noise = 0.05 + 0.5 * uniform(), offset = 2.0 * uniform() - 0.5;
    std::vector<double> y((size_t)T);
    std::vector<float> yf((size_t)T);
    double c = 0.0;
    for (long t = 0; t < T; ++t) {
      c = c * g + (uniform() < 0.05 ? 1.0 : 0.0);
      y[(size_t)t] = c + offset + noise * normal();
      yf[(size_t)t] = (float)y[(size_t)t];
    }
    const int which = i & 1, rounds = 1 + (int)(rng() % 20);
    const double other = (i % 4) >= 2 ? 0.1 * uniform() : 0.0;
    run_trace(y, g, which, noise, other, 0.0, rounds, "random");
    run_trace(yf, g, which, 0.5 * noise, other, 0.1, rounds, "random, float");
    run_trace(y, g, which, 0.0, other, -0.2, rounds, "random, sigma 0");
  }
  {  // what the fit is for: a long trace with an offset of three sigma, a fair threshold
    const long T = 4000;
    const double g = gs[1], noise = 0.2, offset = 0.6;
    std::vector<double> y((size_t)T);
    double c = 0.0;
    for (long t = 0; t < T; ++t) {
      c = c * g + (uniform() < 0.03 ? 1.0 : 0.0);
      y[(size_t)t] = c + offset + noise * normal();
    }
    const std::vector<double> G = table(g, T);
    std::vector<DcPool> pool((size_t)T);
    std::vector<double> cc((size_t)T), a((size_t)T);
    const double b = dc_base_fit_host(y.data(), T, g, G.data(), 0.0, 0.5, 0.0, 8, pool, cc.data(), a.data());
    const int32_t n = dc_base_forward_host(y.data(), T, g, G.data(), 0.0, 0.5, b, pool);
    const DcBaseSums s = dc_base_sums_host(y.data(), T, G.data(), b, pool, n, cc.data(), a.data());
    CHECK(fabs(b - offset) <= 0.5 * noise, "the fit: b = %g for an offset of %g", b, offset);
    CHECK(fabs(s.S / (double)T) <= 0.05 * noise, "the fit: the mean residual %g is not near zero", s.S / (double)T);
  }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("deconv_base_check: ok\n");
  return 0;
}
