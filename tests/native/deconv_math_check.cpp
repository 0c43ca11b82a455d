// Stand-alone host check of the AR(1) deconvolution arithmetic, deep_calcium_amd/csrc/deconv_math.h (dc_deconv_push and the
// functions it is made of, dc_deconv_calcium, dc_deconv_spike), meant to be built with -fsanitize=address,undefined and run as a
// program of its own (tests/test_deconv_api.py does that):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all deconv_math_check.cpp -o check && ./check
// The oracle is a restatement in long double: every merge against the same formula on the same operands, and whole traces
// against a textbook stack of pools (a vector that is pushed and popped), within 1e-12 relative.  The stack the header's step is
// given checks its own bounds: at frame t it may only store into slots 0 .. t - 1 and only load a slot that was stored.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../deep_calcium_amd/csrc/deconv_math.h"

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
static double normal() {                                     // sum of 12 uniforms: good enough for noise
  double s = -6.0;
  for (int i = 0; i < 12; ++i) s += uniform();
  return s;
}

static bool close(ld got, ld want, ld scale) { return fabsl(got - want) <= 1e-12L * (fabsl(want) > scale ? fabsl(want) : scale); }

// The stack below the top pool, with the bounds the kernel's workspace has: T slots, and at frame t only slots below t are live.
struct CheckedStack {
  std::vector<DcPool> slot;
  std::vector<char> written;
  long frame = 0, loads = 0, stores = 0;
  explicit CheckedStack(long T) : slot((size_t)T), written((size_t)T, 0) {}
  DcPool load(int32_t i) {
    CHECK(i >= 0 && i < frame && written[(size_t)i], "load of slot %d at frame %ld", i, frame);
    ++loads;
    return slot.at((size_t)i);
  }
  void store(int32_t i, const DcPool& p) {
    CHECK(i >= 0 && i < (frame > 0 ? frame : 1), "store into slot %d at frame %ld", i, frame);
    ++stores;
    slot.at((size_t)i) = p;
    written.at((size_t)i) = 1;
  }
};

struct WidePool { ld v, w; long t0, l; };

// the textbook form: push, then merge the two highest pools while the higher one is violated
static std::vector<WidePool> wide_forward(const std::vector<double>& y, const std::vector<double>& G, double lam, double smin) {
  const long T = (long)y.size();
  const ld g = G[1];
  std::vector<WidePool> st;
  for (long t = 0; t < T; ++t) {
    const ld mu = t < T - 1 ? (ld)lam * (1.0L - g) : (ld)lam;
    st.push_back({(ld)y[(size_t)t] - mu, 1.0L, t, 1});
    while (st.size() >= 2 && st.back().v < (ld)G[(size_t)st[st.size() - 2].l] * st[st.size() - 2].v + (ld)smin) {
      const WidePool q = st.back();
      st.pop_back();
      WidePool& p = st.back();
      const ld a = G[(size_t)p.l];
      const ld den = p.w + a * a * q.w;
      p.v = (p.w * p.v + a * q.w * q.v) / den;
      p.w = den;
      p.l += q.l;
    }
  }
  return st;
}

static void run_trace(const std::vector<double>& y, double g, double lam, double smin, int expect_pools, const char* what) {
  const long T = (long)y.size();
  std::vector<double> G((size_t)T + 1);
  G[0] = 1.0;
  for (long l = 1; l <= T; ++l) G[(size_t)l] = G[(size_t)l - 1] * g;
  CheckedStack st(T);
  DcPool top = dc_deconv_new(0.0, 0);
  int32_t n = 0;
  double scale = 1.0;
  for (long t = 0; t < T; ++t) {
    st.frame = t;
    scale = fmax(scale, fabs(y[(size_t)t]));
    dc_deconv_push(top, n, st, y[(size_t)t] - dc_deconv_mu(lam, g, t, T), t, G.data(), smin);
    CHECK(n >= 1 && n <= t + 1 && top.t0 + top.l == t + 1, "%s: frame %ld: n = %d, the top pool ends at %d", what, t, n, top.t0 + top.l);
  }
  st.frame = T;
  st.store(n - 1, top);
  CHECK(st.stores <= T && st.loads <= T, "%s: %ld stores and %ld loads for %ld frames", what, st.stores, st.loads, T);
  if (expect_pools >= 0) CHECK(n == expect_pools, "%s: %d pools, not %d", what, n, expect_pools);
  // the pools tile [0, T) in order, with positive weights
  long at = 0;
  for (int32_t i = 0; i < n; ++i) {
    const DcPool p = st.load(i);
    CHECK(p.t0 == at && p.l >= 1 && p.w >= 1.0, "%s: pool %d starts at %d (expected %ld), l = %d, w = %g", what, i, p.t0, at, p.l, p.w);
    at += p.l;
  }
  CHECK(at == T, "%s: the pools cover %ld of %ld frames", what, at, T);
  // against the long double restatement: the calcium always where smin == 0 (it is continuous in the merge decisions), the
  // pools themselves wherever both made the same decisions
  const std::vector<WidePool> want = wide_forward(y, G, lam, smin);
  bool same = (long)want.size() == n;
  for (int32_t i = 0; same && i < n; ++i) same = st.slot[(size_t)i].t0 == want[(size_t)i].t0;
  if (same) {
    for (int32_t i = 0; i < n; ++i)
      CHECK(close(st.slot[(size_t)i].v, want[(size_t)i].v, scale) && close(st.slot[(size_t)i].w, want[(size_t)i].w, 1.0L),
            "%s: pool %d: v = %.17g, w = %.17g", what, i, st.slot[(size_t)i].v, st.slot[(size_t)i].w);
  }
  if (same || smin == 0.0) {
    std::vector<ld> wc((size_t)T);
    for (const WidePool& p : want)
      for (long k = 0; k < p.l; ++k) wc[(size_t)(p.t0 + k)] = (p.v > 0 ? p.v : 0.0L) * (ld)G[(size_t)k];
    for (int32_t i = 0; i < n; ++i) {
      const DcPool& p = st.slot[(size_t)i];
      for (int32_t k = 0; k < p.l; ++k) {
        const double c = dc_deconv_calcium(p.v, G[(size_t)k]);
        CHECK(c >= 0.0 && !signbit(c) && close(c, wc[(size_t)(p.t0 + k)], scale), "%s: calcium[%d] = %.17g", what, p.t0 + k, c);
      }
    }
  }
}

int main() {
  // ---- single operations against long double on the same operands ----
  for (int i = 0; i < 200000; ++i) {
    DcPool p = {normal() * 3, 1.0 + uniform() * 40, 0, 1 + (int32_t)(rng() % 50)};
    DcPool q = {normal() * 3, 1.0 + uniform() * 40, p.l, 1 + (int32_t)(rng() % 50)};
    const double a = exp(-uniform() * 5);
    const DcPool m = dc_deconv_merge(p, q, a);
    const ld den = (ld)p.w + (ld)a * a * q.w, num = (ld)p.w * p.v + (ld)a * q.w * q.v;
    // relative to the larger of the two products: their sum may cancel
    const ld mag = fmaxl(fabsl((ld)p.w * p.v), fabsl((ld)a * q.w * q.v)) / den;
    CHECK(close(m.v, num / den, mag) && close(m.w, den, 1.0L) && m.t0 == p.t0 && m.l == p.l + q.l, "merge %d: v = %.17g", i, m.v);
    const double smin = (i & 1) ? uniform() : 0.0;
    const ld edge = (ld)a * p.v + smin;
    if (fabsl(q.v - edge) > 1e-12L * (1 + fabsl(edge))) CHECK(dc_deconv_violates(p, q, a, smin) == (q.v < edge), "violates %d", i);
    const double c = dc_deconv_calcium(p.v, a);
    CHECK(close(c, (p.v > 0 ? (ld)p.v * a : 0.0L), 1.0L) && !signbit(c), "calcium %d", i);
    CHECK(close(dc_deconv_spike(q.v, a, p.v), (ld)q.v - (ld)a * p.v, fmaxl(fabsl((ld)q.v), fabsl((ld)a * p.v))), "spike %d", i);
  }
  CHECK(dc_deconv_calcium(-1.0, 0.5) == 0.0 && !signbit(dc_deconv_calcium(-1.0, 0.5)) && !signbit(dc_deconv_calcium(-0.0, 0.5)), "+0.0");
  CHECK(dc_deconv_mu(0.25, 0.5, 0, 1) == 0.25 && dc_deconv_mu(0.25, 0.5, 0, 2) == 0.125 && dc_deconv_mu(0.25, 0.5, 1, 2) == 0.25, "mu");

  // ---- structural traces: the deepest stack, the single pool, the cascade ----
  const double gs[] = {exp(-1.0 / 2), exp(-1.0 / 8), exp(-1.0 / 30)};
  for (double g : gs) {
    for (long T : {1L, 2L, 3L, 17L, 200L, 1000L}) {
      std::vector<double> y((size_t)T);
      for (long t = 0; t < T; ++t) y[(size_t)t] = (double)(t + 1);
      run_trace(y, g, 0.0, 0.0, (int)T, "ramp");                       // never merges: depth T
      for (long t = 0; t < T; ++t) y[(size_t)t] = -(double)t;
      run_trace(y, g, 0.0, 0.0, 1, "collapse");                        // merges at every frame
      for (long t = 0; t < T; ++t) y[(size_t)t] = 1.5;
      run_trace(y, g, 0.0, 0.0, -1, "constant");
      run_trace(y, g, 0.3, 0.7, -1, "constant, lam, smin");
      for (long t = 0; t < T; ++t) y[(size_t)t] = t + 1 < T ? (double)(t + 1) : -1e6;
      // the last frame pulls the pools below it down into one for as long as what is left of it, about 1e6 g^k, outweighs the
      // ramp: through all of them at the slowest decay and up to 200 frames
      run_trace(y, g, 0.0, 0.0, g == gs[2] && T <= 200 ? 1 : -1, "cascade");
    }
  }
  // ---- random traces: events on noise ----
  for (int i = 0; i < 300; ++i) {
    const long T = 1 + (long)(rng() % 400);
    const double g = gs[i % 3];
    std::vector<double> y((size_t)T);
    double c = 0.0;
    for (long t = 0; t < T; ++t) {
      c = c * g + (uniform() < 0.05 ? 1.0 : 0.0);
      y[(size_t)t] = c + 0.2 * normal();
    }
    const int mode = i % 4;
    run_trace(y, g, mode == 1 || mode == 3 ? 0.1 + 0.2 * uniform() : 0.0, mode >= 2 ? 0.2 + 0.4 * uniform() : 0.0, -1, "random");
  }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("deconv_math_check: ok\n");
  return 0;
}
