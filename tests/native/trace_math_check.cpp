// Stand-alone host check of the 128-bit helpers the ROI-trace kernels add to deep_calcium_amd/csrc/series_math.h (dc_i128_add,
// dc_i128_from_i64, dc_i128_mul_i64), meant to be built with -fsanitize=address,undefined and run as a program of its own
// (tests/test_traces_api.py does that):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all trace_math_check.cpp -o check && ./check
// The oracle is the compiler's __int128 (unsigned, so that wrapping is defined), over edge values, random values and the
// z-score numerators as csrc/traces.hip forms them at the limit T * H * W = 2^46.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../deep_calcium_amd/csrc/series_math.h"

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

static u128 wide(DcI128 a) { return ((u128)(uint64_t)a.hi << 64) | a.lo; }
static DcI128 narrow(u128 v) {
  DcI128 a;
  a.lo = (uint64_t)v;
  a.hi = (int64_t)(uint64_t)(v >> 64);
  return a;
}
static u128 sext(int64_t b) { return (u128)(i128)b; }

int main() {
  const int64_t e64[] = {0, 1, -1, 2, -2, INT64_MAX, INT64_MIN, INT64_MIN + 1, 0xffffffffll, 0x100000000ll, -0x100000000ll, 2147483647ll,
                         -2147483648ll, 65535ll, 1ll << 46, (1ll << 46) * 65535ll, -(1ll << 46) * 32768ll, (1ll << 62), (1ll << 53) + 1};
  std::vector<int64_t> v64(e64, e64 + sizeof(e64) / sizeof(e64[0]));
  for (int i = 0; i < 300; ++i) v64.push_back((int64_t)(rng() >> (rng() % 64)) * ((rng() & 1) ? 1 : -1));
  std::vector<u128> v128;
  for (int64_t a : v64) {
    v128.push_back(sext(a));
    v128.push_back(sext(a) << 64);
    v128.push_back((sext(a) << 64) | 0xffffffffffffffffull);
    v128.push_back(sext(a) << 32);
  }
  v128.push_back((u128)1 << 127);                        // the most negative value: negation wraps onto itself
  v128.push_back(((u128)1 << 127) - 1);
  v128.push_back(~(u128)0);
  for (int i = 0; i < 300; ++i) v128.push_back((((u128)rng() << 64) | rng()) >> (rng() % 128));

  for (int64_t a : v64) CHECK(wide(dc_i128_from_i64(a)) == sext(a), "from_i64 %lld", (long long)a);
  for (size_t i = 0; i < v128.size(); ++i) {
    const DcI128 a = narrow(v128[i]);
    for (size_t j = 0; j < v128.size(); j += 3) {
      const DcI128 b = narrow(v128[j]);
      CHECK(wide(dc_i128_add(a, b)) == v128[i] + v128[j], "add %zu %zu", i, j);
      CHECK(wide(dc_i128_sub(dc_i128_add(a, b), b)) == v128[i], "add then sub %zu %zu", i, j);
    }
    for (int64_t b : v64)                                // the low 128 bits of the product, for every sign combination
      CHECK(wide(dc_i128_mul_i64(a, b)) == v128[i] * sext(b), "mul_i64 %zu * %lld", i, (long long)b);
  }
  // agrees with the 64 x 64 product where both apply
  for (int64_t a : v64)
    for (int64_t b : v64) CHECK(wide(dc_i128_mul_i64(dc_i128_from_i64(a), b)) == wide(dc_i128_mul(a, b)), "mul_i64 against mul");

  // the z-score of one ROI as traces.hip forms it: T frames, sums S_t with |S_t| <= 65535 * HW, T * HW <= 2^46
  for (int i = 0; i < 20000; ++i) {
    const int64_t hw = 1 + (int64_t)(rng() % (1ull << (rng() % 31)));
    const int64_t tmax = (1ll << 46) / hw;
    const int64_t T = (i & 1) ? tmax : 1 + (int64_t)(rng() % (uint64_t)tmax);
    const int n = 6;                                      // n distinct values, each repeated T / n times (+ the rest on the first)
    DcI128 s2 = {0, 0};
    int64_t s1 = 0;
    i128 w1 = 0, w2 = 0;
    for (int k = 0; k < n; ++k) {
      int64_t S = (int64_t)(rng() % (uint64_t)(hw * 98304 + 1)) - hw * 32768;      // [-32768 hw, 65535 hw + ...]: clip
      if (S > hw * 65535) S = hw * 65535;
      if (i % 7 == 0) S = (k & 1) ? hw * 65535 : -hw * 32768;                        // the extremes
      const int64_t reps = T / n + (k == 0 ? T % n : 0);
      s1 += S * reps;
      s2 = dc_i128_add(s2, dc_i128_mul_i64(dc_i128_mul(S, S), reps));
      w1 += (i128)S * reps;
      w2 += (i128)S * S * reps;
    }
    CHECK((i128)s1 == w1 && wide(s2) == (u128)w2, "sums T=%lld hw=%lld", (long long)T, (long long)hw);
    const DcI128 den = dc_i128_sub(dc_i128_mul_i64(s2, T), dc_i128_mul(s1, s1));
    const i128 wden = (i128)T * w2 - w1 * w1;
    CHECK(wide(den) == (u128)wden && wden >= 0, "denominator T=%lld hw=%lld", (long long)T, (long long)hw);
    const int64_t S0 = hw * 65535;
    const DcI128 num = dc_i128_sub(dc_i128_mul(T, S0), dc_i128_from_i64(s1));
    CHECK(wide(num) == (u128)((i128)T * S0 - w1), "numerator T=%lld hw=%lld", (long long)T, (long long)hw);
  }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("trace_math_check: ok\n");
  return 0;
}
