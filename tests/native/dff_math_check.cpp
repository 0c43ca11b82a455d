// Stand-alone host check of the two helpers of the dF/F baseline kernel, deep_calcium_amd/csrc/dff_math.h (dc_dff_rank,
// dc_dff_midpoint), meant to be built with -fsanitize=address,undefined and run as a program of its own
// (tests/test_dff_api.py does that):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all dff_math_check.cpp -o check && ./check
// The oracle is the compiler's __int128.  The midpoint is taken at the int64 extremes, where lo + hi and hi - lo both overflow
// (the undefined-behaviour sanitizer would stop the program), and the bisection of csrc/dff.hip is run over them to its end.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../deep_calcium_amd/csrc/dff_math.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                     \
  do {                                                       \
    if (!(cond)) {                                           \
      if (++g_fail <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
    }                                                        \
  } while (0)

typedef __int128 i128;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rng() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}

static i128 floor_half(i128 s) { return s >= 0 ? s / 2 : -((-s + 1) / 2); }

// the k-th smallest by the kernel's bisection: the smallest v in [min, max] with #{x <= v} >= k + 1; also counts the rounds
static int64_t bisect(const std::vector<int64_t>& w, int k, int* rounds) {
  int64_t lo = *std::min_element(w.begin(), w.end()), hi = *std::max_element(w.begin(), w.end());
  *rounds = 0;
  while (lo < hi) {
    const int64_t mid = dc_dff_midpoint(lo, hi);
    int c = 0;
    for (int64_t x : w) c += x <= mid ? 1 : 0;
    if (c >= k + 1) hi = mid;
    else lo = mid + 1;
    ++*rounds;
  }
  return lo;
}

int main() {
  const int64_t lim = (1ll << 62) - 1;
  const int64_t e64[] = {0, 1, -1, 2, -2, 3, INT64_MAX, INT64_MAX - 1, INT64_MIN, INT64_MIN + 1, lim, -lim, lim - 1, -lim + 1, 1ll << 62,
                         -(1ll << 62), 0x7fffffffll, 0x80000000ll, -0x80000000ll, 0xffffffffll, 0x100000000ll, (1ll << 53) + 1};
  std::vector<int64_t> v(e64, e64 + sizeof(e64) / sizeof(e64[0]));
  for (int i = 0; i < 400; ++i) v.push_back((int64_t)(rng() >> (rng() % 64)) * ((rng() & 1) ? 1 : -1));
  for (int64_t a : v)
    for (int64_t b : v) {
      const int64_t lo = a < b ? a : b, hi = a < b ? b : a;
      const int64_t mid = dc_dff_midpoint(lo, hi);
      CHECK((i128)mid == floor_half((i128)lo + (i128)hi), "midpoint(%lld, %lld) = %lld", (long long)lo, (long long)hi, (long long)mid);
      CHECK(lo <= mid && mid <= hi && (lo == hi || mid < hi), "midpoint(%lld, %lld) leaves the interval", (long long)lo, (long long)hi);
    }

  // the rank: every q and every window the kernel can meet, against the same rule in 128 bits; monotone, 0 and n - 1 at the ends
  for (int n = 1; n <= 4095; ++n) {
    int prev = 0;
    for (int q = 0; q <= 100; ++q) {
      const int k = dc_dff_rank(q, n);
      CHECK((i128)k == ((i128)q * (n - 1)) / 100, "rank(%d, %d) = %d", q, n, k);
      CHECK(k >= prev && k >= 0 && k < n, "rank(%d, %d) = %d out of order", q, n, k);
      prev = k;
    }
    CHECK(dc_dff_rank(0, n) == 0 && dc_dff_rank(100, n) == n - 1, "rank at the ends, n = %d", n);
  }
  CHECK(dc_dff_rank(29, 101) == 29 && dc_dff_rank(8, 1801) == 144 && dc_dff_rank(100, INT32_MAX) == INT32_MAX - 1, "rank examples");

  // the bisection over windows that span the int64 extremes and the kernel's contract |N| < 2^62, against a sort
  for (int i = 0; i < 3000; ++i) {
    const int n = 1 + (int)(rng() % 40);
    const int mode = i % 4;
    std::vector<int64_t> w(n);
    for (int j = 0; j < n; ++j) {
      if (mode == 0) w[j] = (rng() & 1) ? lim : -lim;                                     // two values 2^63 - 2 apart
      else if (mode == 1) w[j] = (rng() & 1) ? INT64_MAX : INT64_MIN;                     // beyond the contract: still defined
      else if (mode == 2) w[j] = (int64_t)(rng() % 5000) + 1000;
      else w[j] = (int64_t)(rng() >> (rng() % 64)) * ((rng() & 1) ? 1 : -1);
    }
    std::vector<int64_t> s(w);
    std::sort(s.begin(), s.end());
    for (int q = 0; q <= 100; q += (i % 7) + 1) {
      const int k = dc_dff_rank(q, n);
      int rounds = 0;
      const int64_t got = bisect(w, k, &rounds);
      CHECK(got == s[k], "bisection n=%d q=%d: %lld, sorted gives %lld", n, q, (long long)got, (long long)s[k]);
      CHECK(rounds <= 64, "bisection took %d rounds", rounds);
    }
  }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("dff_math_check: ok\n");
  return 0;
}
