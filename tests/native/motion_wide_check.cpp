// Stand-alone host check of the wide-search arithmetic of deep_calcium_amd/csrc/motion_math.h (dc_motion_bin_round,
// dc_motion_centre, dc_motion_cand_around, dc_motion_pick_around_serial), meant to be built with -fsanitize=address,undefined and
// run as a program of its own (tests/test_motion_wide_api.py does that):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all motion_wide_check.cpp -o check && ./check
// The oracles: the floor of the bin by a loop that walks down from the truncated quotient, the centre clamp in 128-bit integers,
// and the order over total shifts by a brute-force minimum of the tuples (score, dy^2 + dx^2, dy, dx) under std::tuple's order.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <tuple>
#include <vector>

#include "../../deep_calcium_amd/csrc/motion_math.h"

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

// floor((sum + n / 2) / n) without a shift: the truncated quotient, stepped down while the remainder is negative
static int bin_ref(long sum, int n) {
  const long a = sum + n / 2;
  long q = a / n;
  while (q * n > a) --q;
  return (int)q;
}

typedef std::tuple<int64_t, unsigned __int128, int, int> Key;
static Key key(const DcShiftCand c) { return Key(c.score, (unsigned __int128)((__int128)c.dy * c.dy + (__int128)c.dx * c.dx), c.dy, c.dx); }

int main() {
  // 1. the rounding rule of the bin: every sum a c x c cell of 16-bit values can have at c = 2, a sweep and the extremes at 4, 8
  CHECK(dc_motion_bin_log2(2) == 1 && dc_motion_bin_log2(4) == 2 && dc_motion_bin_log2(8) == 3, "log2");
  for (int c : {0, 1, 3, 5, 6, 7, 9, 16, -2, -4}) CHECK(dc_motion_bin_log2(c) == -1, "log2 of %d", c);
  CHECK(dc_motion_bin_round(-1 - 1 - 1 - 2, 1) == -1, "[-1, -1, -1, -2] at c = 2 gives -1");        // (-5 + 2) / 4 = -0.75 -> -1
  CHECK(dc_motion_bin_round(-6, 1) == -1 && dc_motion_bin_round(-7, 1) == -2 && dc_motion_bin_round(-2, 1) == 0, "halves round up");
  CHECK(dc_motion_bin_round(2, 1) == 1 && dc_motion_bin_round(1, 1) == 0 && dc_motion_bin_round(-3, 1) == -1, "halves round up");
  for (int lg = 1; lg <= 3; ++lg) {
    const int n = 1 << (2 * lg);
    const long lo = -32768L * n, hi = 65535L * n;
    CHECK(dc_motion_bin_round((int)lo, lg) == -32768 && dc_motion_bin_round((int)hi, lg) == 65535, "an all-extreme cell keeps its value");
    CHECK(dc_motion_bin_round(32767 * n, lg) == 32767 && dc_motion_bin_round(0, lg) == 0, "constant cells");
    const long step = lg == 1 ? 1 : 7;
    for (long s = lo; s <= hi; s += step) CHECK(dc_motion_bin_round((int)s, lg) == bin_ref(s, n), "bin %ld lg %d", s, lg);
    for (long s = -3 * n; s <= 3 * n; ++s) CHECK(dc_motion_bin_round((int)s, lg) == bin_ref(s, n), "bin %ld lg %d", s, lg);
    // the mean of values between a and b lies between them
    for (int trial = 0; trial < 2000; ++trial) {
      long sum = 0;
      int mn = 70000, mx = -70000;
      for (int i = 0; i < n; ++i) {
        const int v = (int)(rng() % 98304) - 32768;
        sum += v; mn = std::min(mn, v); mx = std::max(mx, v);
      }
      const int b = dc_motion_bin_round((int)sum, lg);
      CHECK(b >= mn && b <= mx, "bin %d outside [%d, %d]", b, mn, mx);
    }
  }

  // 2. the centre clamp, with mult * row far beyond int32
  const int rows[] = {0, 1, -1, 3, -3, 15, -15, 16, -16, 17, 1000, -1000, 2147483647, -2147483647 - 1, 2147483646, -2147483647};
  const int mults[] = {0, 1, 2, 4, 8, -8, 2147483647, -2147483647 - 1};
  const int Ms[] = {0, 1, 4, 14, 120, 128};
  for (int row : rows)
    for (int mult : mults)
      for (int M : Ms) {
        const __int128 v = (__int128)mult * row;
        const int want = v < -M ? -M : (v > M ? M : (int)v);
        CHECK(dc_motion_centre(mult, row, M) == want, "centre %d * %d within %d", mult, row, M);
      }
  CHECK(dc_motion_centre(8, 2147483647, 120) == 120 && dc_motion_centre(8, -2147483647 - 1, 120) == -120, "the int32 extremes clamp");
  CHECK(dc_motion_centre(4, 3, 20) == 12 && dc_motion_centre(4, -6, 20) == -20 && dc_motion_centre(4, 5, 20) == 20, "clamp at +-(S - D)");

  // 3. the order over TOTAL shifts: the named tie, then random tables against the brute-force minimum
  {
    const int D = 2, nd = 5;
    std::vector<int64_t> sc((size_t)(nd * nd), 100);
    sc[(size_t)((-2 + D) * nd + D)] = 7;                 // residual (-2, 0): total (2, 0)
    sc[(size_t)((1 + D) * nd + D)] = 7;                  // residual (1, 0): total (5, 0)
    const DcShiftCand b = dc_motion_pick_around_serial(sc.data(), D, 4, 0);
    CHECK(b.dy == 2 && b.dx == 0 && b.score == 7, "the tie goes to the smallest TOTAL displacement: (%d, %d)", b.dy, b.dx);
    const DcShiftCand r = dc_motion_pick_serial(sc.data(), D);
    CHECK(r.dy == 1 && r.dx == 0, "an order over residuals would pick the residual (1, 0), the total (5, 0)");
  }
  for (int trial = 0; trial < 4000; ++trial) {
    const int D = (int)(rng() % 9), nd = 2 * D + 1, n = nd * nd;
    const int cy = (int)(rng() % 257) - 128, cx = (trial % 5 == 0) ? 0 : (int)(rng() % 257) - 128;
    std::vector<int64_t> sc((size_t)n);
    const int mode = trial % 4;                          // 0: random, 1: two values, 2: constant, 3: extremes
    for (int i = 0; i < n; ++i) {
      if (mode == 0) sc[(size_t)i] = (int64_t)(rng() % 1000000);
      else if (mode == 1) sc[(size_t)i] = (int64_t)(rng() % 2) * 5 + 3;
      else if (mode == 2) sc[(size_t)i] = 42;
      else sc[(size_t)i] = (rng() & 1) ? (((int64_t)1 << 62) - 1) : (int64_t)(rng() >> 2);
    }
    std::vector<DcShiftCand> all;
    for (int i = 0; i < n; ++i) {
      const DcShiftCand c = dc_motion_cand_around(sc.data(), D, i, cy, cx);
      CHECK(c.score == sc[(size_t)i] && c.dy == cy + i / nd - D && c.dx == cx + i % nd - D, "cand %d", i);
      all.push_back(c);
    }
    DcShiftCand want = all[0];
    for (const DcShiftCand c : all)
      if (key(c) < key(want)) want = c;
    const DcShiftCand got = dc_motion_pick_around_serial(sc.data(), D, cy, cx);
    CHECK(key(got) == key(want), "serial pick D=%d trial=%d", D, trial);
    if (mode == 2) {                                     // constant scores: the candidate of the window nearest (0, 0), per axis
      const int wy = cy > D ? cy - D : (cy < -D ? cy + D : 0), wx = cx > D ? cx - D : (cx < -D ? cx + D : 0);
      CHECK(got.dy == wy && got.dx == wx, "constant scores pick (%d, %d), not (%d, %d)", wy, wx, got.dy, got.dx);
    }
    // 64 strided partial minima, folded by a butterfly (what the kernel does)
    DcShiftCand part[64];
    for (int l = 0; l < 64; ++l) {
      part[l] = all[(size_t)(l < n ? l : 0)];
      for (int i = l + 64; i < n; i += 64)
        if (dc_motion_before(all[(size_t)i], part[l])) part[l] = all[(size_t)i];
    }
    for (int o = 32; o > 0; o >>= 1) {
      DcShiftCand next[64];
      for (int l = 0; l < 64; ++l) next[l] = dc_motion_before(part[l ^ o], part[l]) ? part[l ^ o] : part[l];
      for (int l = 0; l < 64; ++l) part[l] = next[l];
    }
    for (int l = 0; l < 64; ++l) CHECK(key(part[l]) == key(want), "butterfly lane %d", l);
  }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("motion_wide_check: ok\n");
  return 0;
}
