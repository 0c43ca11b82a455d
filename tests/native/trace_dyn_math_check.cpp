// Stand-alone host check of the trace-dynamics arithmetic, deep_calcium_amd/csrc/trace_dyn_math.h (the order key, the medians, the
// fixed-order fold, the autocovariance and the decay), meant to be built with -fsanitize=address,undefined and run as a program
// of its own (tests/test_dynamics_api.py does that):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all trace_dyn_math_check.cpp -o check && ./check
// The oracles are restatements: the medians against a full sort, and against the 8-bit radix descent over the key that the
// device kernel walks (emulated here on the host, so that descent is checked against values too); the fold against a long double
// sum within its rounding bound; the decay against long double on the same operands.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
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

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}
static double uniform() { return (double)(rng() >> 11) * (1.0 / 9007199254740992.0); }
static double normal() {
  double s = -6.0;
  for (int i = 0; i < 12; ++i) s += uniform();
  return s;
}
static uint64_t bits(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }

// the k-th smallest key by the kernel's descent: eight passes of 256 counters
static uint64_t radix_select(const std::vector<uint64_t>& keys, size_t k, size_t* le) {
  uint64_t prefix = 0;
  size_t below = 0, count = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    std::vector<size_t> hist(256, 0);
    for (uint64_t key : keys)
      if (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8))) ++hist.at((size_t)((key >> shift) & 255u));
    size_t excl = 0;
    for (size_t b = 0; b < 256; ++b) {
      if (excl <= k && k < excl + hist[b]) {
        prefix |= (uint64_t)b << shift;
        k -= excl;
        below += excl;
        count = hist[b];
        break;
      }
      excl += hist[b];
    }
  }
  *le = below + count;
  return prefix;
}

static double radix_median(const std::vector<double>& x) {
  std::vector<uint64_t> keys;
  for (double v : x) keys.push_back(dc_dyn_key(v));
  const size_t n = x.size(), k = (n - 1) / 2;
  size_t le;
  const uint64_t lo = radix_select(keys, k, &le);
  if (n & 1) return dc_dyn_unkey(lo);
  uint64_t hi = lo;
  if (le <= k + 1) {
    hi = ~0ull;
    for (uint64_t key : keys)
      if (key > lo && key < hi) hi = key;
  }
  return dc_dyn_mid(dc_dyn_unkey(lo), dc_dyn_unkey(hi));
}

static double sorted_median(std::vector<double> x) {
  std::sort(x.begin(), x.end());
  const size_t n = x.size();
  return (n & 1) ? x[(n - 1) / 2] : (x[n / 2 - 1] + x[n / 2]) / 2.0;
}

int main() {
  // ---- the key orders doubles as numbers and comes back unchanged ----
  const double special[] = {-INFINITY, -1e300, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1e300, INFINITY};
  for (size_t i = 0; i + 1 < sizeof(special) / sizeof(special[0]); ++i)
    CHECK(dc_dyn_key(special[i]) < dc_dyn_key(special[i + 1]), "key order at %zu", i);
  for (int i = 0; i < 200000; ++i) {
    const double a = normal() * exp(20 * normal()), b = (i & 3) ? normal() * exp(20 * normal()) : a;
    CHECK(bits(dc_dyn_unkey(dc_dyn_key(a))) == bits(a), "key round trip of %.17g", a);
    CHECK((a < b) == (dc_dyn_key(a) < dc_dyn_key(b)) && (a == b) == (dc_dyn_key(a) == dc_dyn_key(b)), "key order of %.17g, %.17g", a, b);
  }
  // ---- medians: nth_element, the radix descent and a full sort agree in value, ties and both parities included ----
  for (int i = 0; i < 3000; ++i) {
    const size_t n = 1 + (size_t)(rng() % 600);
    std::vector<double> x(n);
    const int mode = i % 3;
    for (double& v : x) v = mode == 0 ? normal() : mode == 1 ? (double)(rng() % 8) / 4.0 - 1.0 : ((rng() & 1) ? 0.0 : -0.0);
    const double want = sorted_median(x), radix = radix_median(x);
    std::vector<double> scratch = x;
    const double got = dc_dyn_median_host(scratch);
    CHECK(got == want && radix == want, "median of %zu values (mode %d): %.17g, radix %.17g, sorted %.17g", n, mode, got, radix, want);
  }
  // ---- the noise of whole traces: T < 3, both parities, float and double, a constant trace ----
  std::vector<double> buf;
  for (long T : {1L, 2L, 3L, 4L, 7L, 256L, 257L, 1000L}) {
    std::vector<float> y((size_t)T);
    for (float& v : y) v = (float)normal();
    const double s = dc_dyn_noise_host(y.data(), T, buf);
    std::vector<double> d;
    for (long t = 0; t + 1 < T; ++t) d.push_back((double)y[(size_t)t + 1] - (double)y[(size_t)t]);
    double want = 0.0;
    if (T >= 3) {
      const double m = sorted_median(d);
      for (double& v : d) v = fabs(v - m);
      want = 1.4826 * sorted_median(d) / sqrt(2.0);
    }
    CHECK(bits(s) == bits(want), "noise at T = %ld: %.17g, not %.17g", T, s, want);
    std::vector<double> c((size_t)T, 1.5);
    CHECK(bits(dc_dyn_noise_host(c.data(), T, buf)) == bits(0.0), "noise of a constant trace at T = %ld", T);
  }
  // ---- the fold against long double within its bound; the order is the lanes, then the tree ----
  for (long n : {-3L, 0L, 1L, 2L, 255L, 256L, 257L, 511L, 513L, 5000L}) {
    std::vector<double> f((size_t)(n > 0 ? n : 0));
    ld exact = 0, mag = 0;
    for (double& v : f) { v = normal() * 1e3; exact += v; mag += fabsl((ld)v); }
    const double got = dc_dyn_fold_host([&](long t) { return f.at((size_t)t); }, n);
    const ld bound = (ld)((n + 255) / 256 + 9) * 0x1p-53L * mag;
    CHECK(fabsl((ld)got - exact) <= bound + 0x1p-60L * mag, "fold of %ld terms: %.17g against %.17Lg", n, got, exact);
    if (n <= 0) CHECK(bits(got) == bits(0.0), "the empty fold is +0.0");
    // the same order, written out
    double P[256];
    for (int j = 0; j < 256; ++j) { P[j] = 0.0; for (long t = j; t < n; t += 256) P[j] = P[j] + f[(size_t)t]; }
    for (int h = 128; h >= 1; h /= 2) for (int j = 0; j < h; ++j) P[j] = P[j] + P[j + h];
    CHECK(bits(got) == bits(P[0]), "fold order at n = %ld", n);
  }
  // ---- autocovariance and decay: an AR(1) process comes back; shifting the trace by a constant that keeps the sums exact does not move it ----
  for (int lags : {1, 2, 5, 16}) {
    for (long T : {1L, 3L, 6L, 7L, 18L, 300L, 4000L}) {
      std::vector<double> y((size_t)T);
      double c = 0.0;
      for (double& v : y) { c = 0.9 * c + normal(); v = c; }
      std::vector<double> xc((size_t)lags + 1, -1.0);
      dc_dyn_autocov_host(y.data(), T, lags, xc.data());
      ld mean = 0;
      for (double v : y) mean += v;
      mean /= T;
      for (int l = 0; l <= lags; ++l) {
        ld q = 0, mag = 0;
        for (long t = 0; t + l < T; ++t) { const ld p = ((ld)y[(size_t)t] - mean) * ((ld)y[(size_t)(t + l)] - mean); q += p; mag += fabsl(p); }
        CHECK(fabsl((ld)xc[(size_t)l] - q / T) <= 1e-11L * (mag / T + 1e-300L), "xc[%d] at T = %ld: %.17g against %.17Lg", l, T, xc[(size_t)l], q / T);
      }
      const double g = dc_dyn_decay(xc.data(), lags, 0.0, T);
      if (T < lags + 2) CHECK(isnan(g), "decay at T = %ld, lags = %d is defined: %g", T, lags, g);
      else {
        ld num = 0, den = 0;
        for (int i = 0; i < lags; ++i) { num += (ld)xc[(size_t)i] * xc[(size_t)i + 1]; den += (ld)xc[(size_t)i] * xc[(size_t)i]; }
        CHECK(fabsl((ld)g - num / den) <= 1e-12L * (1 + fabsl(num / den)), "decay at T = %ld, lags = %d: %.17g", T, lags, g);
        if (T == 4000) CHECK(fabs(g - 0.9) < 0.05, "AR(1) with g = 0.9 estimated as %g (lags %d)", g, lags);
      }
    }
  }
  const double flat[3] = {0.0, 0.0, 0.0};
  CHECK(isnan(dc_dyn_decay(flat, 2, 0.0, 100)), "a zero denominator is undefined");
  const double huge[2] = {1e-200, 1e200};
  CHECK(isnan(dc_dyn_decay(huge, 1, 0.0, 100)), "a quotient that is not finite is undefined");
  CHECK(bits(dc_dyn_sigma(1.0)) == bits(1.4826 / sqrt(2.0)) && bits(dc_dyn_mid(1.0, 2.0)) == bits(1.5), "sigma and mid");
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("trace_dyn_math_check: ok\n");
  return 0;
}
