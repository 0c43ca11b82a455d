// Stand-alone host check of the AR(2) deconvolution, deep_calcium_amd/csrc/deconv_ar2_math.h (the push / merge step, the outputs
// and the host forward pass and search built on them), meant to be built with -fsanitize=address,undefined and run as a program of
// its own (tests/test_deconv_ar2_api.py does that):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all deconv_ar2_check.cpp -o check && ./check
// (1) The structural traces: the ramp t + 1 keeps T pools (a stack of depth T, in T entries), -t ends as one pool with calcium and
// spikes all +0.0, and T = 1.  (2) Random traces of ragged length, float and double, in buffers exactly T long, tables exactly
// T + 1 long: a read or write past a trace or a table is the sanitizer's.  The moments A and B of every final pool against the
// direct sums of its frames, v against the least-squares value given u, the pools tile the trace, calcium >= 0 and the spikes
// above rounding.  (3) The search: RSS(p*) recomputed is the one reported and within the target.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../deep_calcium_amd/csrc/deconv_ar2_math.h"

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

// the three rows, each exactly T + 1 long and an allocation of its own
struct Table {
  std::vector<double> h, HH, HP;
  double g1, g2;
  Table(double d, double r, long T) : h((size_t)T + 1), HH((size_t)T + 1), HP((size_t)T + 1), g1(d + r), g2(-(d * r)) {
    h[0] = 1.0;
    if (T >= 1) h[1] = g1;
    for (long k = 2; k <= T; ++k) h[(size_t)k] = g1 * h[(size_t)k - 1] + g2 * h[(size_t)k - 2];
    HH[0] = HP[0] = 0.0;
    for (long l = 0; l < T; ++l) {
      HH[(size_t)l + 1] = HH[(size_t)l] + h[(size_t)l] * h[(size_t)l];
      HP[(size_t)l + 1] = HP[(size_t)l] + (l >= 1 ? h[(size_t)l] * h[(size_t)l - 1] : 0.0);
    }
  }
  DcAr2 model() const {
    DcAr2 m;
    m.g1 = g1;
    m.g2 = g2;
    m.h = h.data();
    m.HH = HH.data();
    m.HP = HP.data();
    return m;
  }
};

static const double kRoots[][2] = {{0.75, 0.25}, {exp(-1.0 / 8), exp(-1.0 / 2)}, {0.99, 0.9}, {0.5, 0.01}};

static bool is_plus_zero(double x) { return x == 0.0 && !signbit(x); }

static void structural(double d, double r, long T) {
  const Table tab(d, r, T);
  const DcAr2 m = tab.model();
  CHECK(dc_ar2_roots_ok(m.g1, m.g2), "roots %g, %g refused", d, r);
  std::vector<DcPool2> pool((size_t)T);
  std::vector<double> y((size_t)T), c((size_t)T), s((size_t)T);
  for (long t = 0; t < T; ++t) y[(size_t)t] = (double)t + 1.0;
  int32_t n = dc_forward_host(y.data(), T, m, 0.0, 0.0, 0.0, pool);
  CHECK(n == T, "roots %g, %g: the ramp of %ld frames kept %d pools", d, r, T, n);
  dc_calcium_host(pool, n, m, c.data());
  dc_spikes_host(pool, n, m, T, c.data(), s.data());
  for (long t = 0; t < T; ++t) CHECK(c[(size_t)t] == y[(size_t)t] && (t == 0 ? is_plus_zero(s[0]) : s[(size_t)t] > 0.0), "the ramp, frame %ld", t);
  for (long t = 0; t < T; ++t) y[(size_t)t] = -(double)t;
  n = dc_forward_host(y.data(), T, m, 0.0, 0.0, 0.0, pool);
  CHECK(n == 1 && pool[0].t0 == 0 && pool[0].l == T, "roots %g, %g: -t of %ld frames ends as %d pools", d, r, T, n);
  dc_calcium_host(pool, n, m, c.data());
  dc_spikes_host(pool, n, m, T, c.data(), s.data());
  for (long t = 0; t < T; ++t) CHECK(is_plus_zero(c[(size_t)t]) && is_plus_zero(s[(size_t)t]), "-t, frame %ld: %g, %g", t, c[(size_t)t], s[(size_t)t]);
}

template <typename In>
static void run_trace(const std::vector<In>& y, double d, double r, double lam, double smin, double b, const char* what) {
  const long T = (long)y.size();
  const Table tab(d, r, T);
  const DcAr2 m = tab.model();
  std::vector<DcPool2> pool((size_t)T);
  std::vector<double> c((size_t)T), s((size_t)T), x((size_t)T);
  const int32_t n = dc_forward_host(y.data(), T, m, lam, smin, b, pool);
  CHECK(n >= 1 && n <= T, "%s: %d pools of %ld frames", what, n, T);
  double top = 0.0;
  for (long t = 0; t < T; ++t) {
    x[(size_t)t] = dc_base_data((double)y[(size_t)t], b) - dc_ar2_mu(lam, m.g1, m.g2, t, T);
    top = fmax(top, fabs((double)y[(size_t)t]));
  }
  dc_calcium_host(pool, n, m, c.data());
  dc_spikes_host(pool, n, m, T, c.data(), s.data());
  int32_t next = 0;
  for (int32_t i = 0; i < n; ++i) {
    const DcPool2& p = pool[(size_t)i];
    CHECK(p.t0 == next && p.l >= 1, "%s: pool %d starts at %d, not %d", what, i, p.t0, next);
    next = p.t0 + p.l;
    long double A = 0.0L, B = 0.0L, scale = 0.0L;
    for (int32_t k = 0; k < p.l; ++k) {
      A += (long double)m.h[k] * x[(size_t)(p.t0 + k)];
      if (k >= 1) B += (long double)m.h[k - 1] * x[(size_t)(p.t0 + k)];
      scale += fabsl((long double)m.h[k] * x[(size_t)(p.t0 + k)]);
    }
    const long double tol = 1e-10L * (scale + 1.0L) * (1.0L + p.l);
    CHECK(fabsl(A - p.A) <= tol && fabsl(B - p.B) <= tol, "%s: pool %d of %d frames: A %g against %Lg, B %g against %Lg", what, i, p.l, p.A, A, p.B, B);
    const double u = i == 0 ? 0.0 : c[(size_t)p.t0 - 1];
    CHECK(p.u == u && (i > 0 || is_plus_zero(p.u)), "%s: pool %d: u = %g, the calcium below is %g", what, i, p.u, u);
    CHECK(p.v == dc_ar2_fit(m, p.A, p.u, p.l), "%s: pool %d: v is not the fit", what, i);
  }
  CHECK(next == T, "%s: the pools end at %d of %ld", what, next, T);
  for (long t = 0; t < T; ++t) {
    CHECK(c[(size_t)t] >= -1e-9 * (top + 1.0), "%s: calcium[%ld] = %g", what, t, c[(size_t)t]);
    CHECK(s[(size_t)t] >= -1e-9 * (top + 1.0), "%s: spikes[%ld] = %g", what, t, s[(size_t)t]);
  }
}

template <typename In>
static void run_search(const std::vector<In>& y, double d, double r, int which, double sigma, double other, int rounds, const char* what) {
  const long T = (long)y.size();
  const Table tab(d, r, T);
  const DcAr2 m = tab.model();
  std::vector<DcPool2> pool((size_t)T);
  std::vector<double> c((size_t)T);
  double param = -1.0, rss = -1.0;
  int32_t status = -1;
  dc_search_host(y.data(), T, m, which, sigma, other, rounds, pool, c.data(), &param, &rss, &status);
  const double target = dc_search_target(sigma, T);
  auto at = [&](double p) {
    const int32_t n = which == DC_SEARCH_LAM ? dc_forward_host(y.data(), T, m, p, other, 0.0, pool) : dc_forward_host(y.data(), T, m, other, p, 0.0, pool);
    return dc_rss_host(y.data(), T, m, pool, n, c.data());
  };
  const double r0 = at(0.0);
  CHECK(status >= 0 && status <= 2 && param >= 0.0 && at(param) == rss, "%s: status %d, p* = %g, RSS reported as %g", what, status, param, rss);
  CHECK((status == 1) == !(r0 < target), "%s: status %d with RSS(0) = %g, target %g", what, status, r0, target);
  if (status == 1) CHECK(param == 0.0, "%s: status 1 with p* = %g", what, param);
  else CHECK(rss <= target, "%s: RSS(p*) = %g is over the target %g", what, rss, target);
}

int main() {
  CHECK(!dc_ar2_roots_ok(1.0, -0.25) && !dc_ar2_roots_ok(1.0, -0.5) && !dc_ar2_roots_ok(1.0, 0.1) && !dc_ar2_roots_ok(-0.5, -0.1) &&
            !dc_ar2_roots_ok(1.5, -0.4) && !dc_ar2_roots_ok(NAN, -0.1) && !dc_ar2_roots_ok(1.0, NAN),
        "roots that are equal, complex, negative, outside (0, 1) or NaN must be refused");
  CHECK(dc_ar2_mu(2.0, 1.0, -0.1875, 0, 1) == 2.0 && dc_ar2_mu(2.0, 1.0, -0.1875, 0, 2) == 0.0 && dc_ar2_mu(2.0, 1.0, -0.1875, 0, 3) == 0.375, "mu");
  for (const auto& dr : kRoots)
    for (long T : {1L, 2L, 3L, 64L, 700L}) structural(dr[0], dr[1], T);

  for (int i = 0; i < 200; ++i) {
    const long T = 1 + (long)(rng() % 500);
    const double d = kRoots[i % 4][0], r = kRoots[i % 4][1], noise = 0.05 + 0.5 * uniform();
    std::vector<double> y((size_t)T);
    std::vector<float> yf((size_t)T);
    double c1 = 0.0, c2 = 0.0;
    for (long t = 0; t < T; ++t) {
      const double c0 = (d + r) * c1 - (d * r) * c2 + (uniform() < 0.05 ? 1.0 : 0.0);
      c2 = c1;
      c1 = c0;
      y[(size_t)t] = c0 * (1.0 - r / d) + noise * normal();
      yf[(size_t)t] = (float)y[(size_t)t];
    }
    const double lam = (i % 4) >= 2 ? 0.2 * uniform() : 0.0, smin = (i % 3) ? noise * 2.0 * uniform() : 0.0;
    run_trace(y, d, r, lam, smin, 0.0, "random");
    run_trace(yf, d, r, lam, smin, 0.1 * normal(), "random, float, baseline");
    const int which = i & 1, rounds = 1 + (int)(rng() % 20);
    run_search(y, d, r, which, noise, which ? smin : lam, rounds, "search");
    run_search(yf, d, r, which, 0.0, 0.0, rounds, "search, sigma 0");
  }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("deconv_ar2_check: ok\n");
  return 0;
}
