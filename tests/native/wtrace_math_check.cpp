// Stand-alone host check of deep_calcium_amd/csrc/wtrace_math.h (the scalar arithmetic of the weighted ROI sums), meant to be built
// with -fsanitize=address,undefined and run as a program of its own (tests/test_weighted_api.py does that):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all wtrace_math_check.cpp -o check && ./check
// The oracle is the compiler's __int128.  Three things: one term at every corner of (weight, pixel) and on random pairs, with what
// 32 bits hold of it; a row AT THE BOUND -- 2^30 entries of weight 65535 over pixels 65535 or -32768 -- summed the way the kernel
// does (64 lanes, pieces of 2048, lane partials, a wave reduction, the running total), every partial sum inside int64 and the total
// below 2^62; and the promises handed to the entry points that take the weight sum for an area.
#include <stdio.h>
#include <stdlib.h>

#include "../../deep_calcium_amd/csrc/wtrace_math.h"

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

// n entries of weight w over pixels all x, summed as the kernel sums them: lane l of 64 takes entries l, l + 64, ... of every piece
// of 2048, the lanes' int64 partials are added (the wave reduction), the piece is added to the running total.  Pieces of equal
// content are folded: `pieces` whole ones and a last one of `rest` entries.
static int64_t kernel_order_sum(int64_t n, int w, int x, int64_t* largest_partial) {
  const int64_t pieces = n / 2048, rest = n % 2048;
  int64_t total = 0, peak = 0;
  for (int pass = 0; pass < 2; ++pass) {
    const int64_t m = pass == 0 ? 2048 : rest, times = pass == 0 ? pieces : (rest ? 1 : 0);
    if (!times) continue;
    int64_t wave = 0;
    for (int lane = 0; lane < 64; ++lane) {
      int64_t v = 0;
      for (int64_t i = lane; i < m; i += 64) v += dc_wtrace_term(w, x);
      if (llabs(v) > peak) peak = llabs(v);
      wave += v;
      if (llabs(wave) > peak) peak = llabs(wave);
    }
    for (int64_t k = 0; k < (times < 4 ? times : 4); ++k) total += wave;         // the first few for real,
    if (times > 4) total += (times - 4) * wave;                                   // the rest at once: same value, checked below
    if (llabs(total) > peak) peak = llabs(total);
  }
  *largest_partial = peak;
  return total;
}

int main() {
  // ---- one term ----
  const int ws[5] = {0, 1, 256, 32768, 65535};
  const int xs[7] = {-32768, -1, 0, 1, 32767, 32768, 65535};
  for (int i = 0; i < 5; ++i)
    for (int j = 0; j < 7; ++j) CHECK((i128)dc_wtrace_term(ws[i], xs[j]) == (i128)ws[i] * xs[j], "term %d x %d", ws[i], xs[j]);
  for (int it = 0; it < 200000; ++it) {
    const int w = (int)(rng() % 65536), x = (int)(rng() % 98304) - 32768;         // the union of both pixel types
    CHECK((i128)dc_wtrace_term(w, x) == (i128)w * x, "term %d x %d", w, x);
  }
  // what 32 bits hold: one worst term of an int16 frame and not two; not even one of a uint16 frame
  CHECK(dc_wtrace_term(65535, -32768) == -2147450880LL && dc_wtrace_term(65535, -32768) >= -2147483647LL - 1, "the int16 corner fits int32");
  CHECK(2 * dc_wtrace_term(65535, -32768) < -2147483647LL - 1, "two int16 corners do not");
  CHECK(dc_wtrace_term(65535, 65535) == 4294836225LL && dc_wtrace_term(65535, 65535) > 2147483647LL, "the uint16 corner does not fit int32");
  CHECK(dc_wtrace_int32_terms(0) == 1 && dc_wtrace_int32_terms(1) == 0, "int32 terms");
  CHECK(2048LL * 65535 < (1LL << 27), "the unweighted piece bound");
  // ---- a row at the bound ----
  const int64_t N = DC_WTRACE_MAX_ENTRIES;
  CHECK(N == (1LL << 30), "DC_WTRACE_MAX_ENTRIES");
  CHECK((i128)dc_wtrace_row_bound(N) == (i128)N * 65535 * 65535 && dc_wtrace_row_bound(N) < (1LL << 62), "row bound below 2^62");
  const int64_t lens[6] = {1, 63, 2049, 1000003, N - 1, N};
  const int px[3] = {65535, -32768, 32767};
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 3; ++j) {
      int64_t peak = 0;
      const int64_t got = kernel_order_sum(lens[i], 65535, px[j], &peak);
      CHECK((i128)got == (i128)lens[i] * 65535 * px[j], "row of %lld entries over %d", (long long)lens[i], px[j]);
      CHECK(peak <= dc_wtrace_row_bound(lens[i]) && peak < (1LL << 62), "a partial sum leaves the row bound (%lld entries)", (long long)lens[i]);
    }
  // ---- the weight sum as an area ----
  CHECK(dc_wtrace_wsum_check(0, 10) == 1 && dc_wtrace_wsum_check(-3, 10) == 1, "W < 1");
  CHECK(dc_wtrace_wsum_check(2147483647LL, 1) == 0 && dc_wtrace_wsum_check(2147483648LL, 1) == 2, "W and 2^31 - 1");
  CHECK(dc_wtrace_wsum_check(1LL << 26, 1LL << 20) == 0 && dc_wtrace_wsum_check((1LL << 26) + 1, 1LL << 20) == 3, "T W and 2^46");
  CHECK(DC_WTRACE_MAX_VOLUME == (1LL << 46) && DC_WTRACE_MAX_WSUM == (1LL << 31) - 1, "limits");
  for (int it = 0; it < 100000; ++it) {                                          // |S| <= 65535 W, term by term
    const int n = 1 + (int)(rng() % 40);
    i128 S = 0, W = 0;
    const bool uns = rng() & 1;
    for (int e = 0; e < n; ++e) {
      const int w = (int)(rng() % 65536), x = uns ? (int)(rng() % 65536) : (int)(rng() % 65536) - 32768;
      S += dc_wtrace_term(w, x);
      W += w;
    }
    CHECK((S < 0 ? -S : S) <= 65535 * W, "|S| <= 65535 W");
  }
  if (g_fail) {
    printf("wtrace_math_check: %d FAILED\n", g_fail);
    return 1;
  }
  printf("wtrace_math_check: ok\n");
  return 0;
}
