// Stand-alone host check of the tie rule of deep_calcium_amd/csrc/motion_math.h (dc_motion_before, dc_motion_cand,
// dc_motion_pick_serial), meant to be built with -fsanitize=address,undefined and run as a program of its own
// (tests/test_motion_api.py does that):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all motion_math_check.cpp -o check && ./check
// The oracle is a brute-force sort of the tuples (score, dy^2 + dx^2, dy, dx) with std::tuple's lexicographic order, over random
// scores, heavily tied scores and the int64 extremes.
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

typedef std::tuple<int64_t, unsigned __int128, int, int> Key;
static Key key(const DcShiftCand c) { return Key(c.score, (unsigned __int128)((__int128)c.dy * c.dy + (__int128)c.dx * c.dx), c.dy, c.dx); }

int main() {
  // 1. the comparison is the tuple order, for every pair of a mixed bag of candidates (equal ones included)
  std::vector<DcShiftCand> bag;
  const int64_t sv[] = {0, 1, -1, 10, 11, INT64_MAX, INT64_MIN, (int64_t)1 << 62, 4611686014132420609ll /* 2^30 * 65535^2 */};
  const int dv[] = {0, 1, -1, 3, -3, 4, -4, 5, -5, 16, -16, 2147483647, -2147483647 - 1};
  for (int64_t s : sv)
    for (int dy : dv)
      for (int dx : dv) bag.push_back(DcShiftCand{s, dy, dx});
  for (size_t i = 0; i < bag.size(); ++i)
    for (size_t j = 0; j < bag.size(); j += 1 + (i % 3)) {
      const bool want = key(bag[i]) < key(bag[j]);
      CHECK(dc_motion_before(bag[i], bag[j]) == want, "before %zu %zu", i, j);
      if (i == j) CHECK(!dc_motion_before(bag[i], bag[j]), "irreflexive %zu", i);
    }
  // (3, 4) and (5, 0) and (0, 5) are equally far: dy decides, then dx
  CHECK(dc_motion_before(DcShiftCand{7, 0, -5}, DcShiftCand{7, 0, 5}), "(0,-5) before (0,5)");
  CHECK(dc_motion_before(DcShiftCand{7, -5, 0}, DcShiftCand{7, -4, -3}), "(-5,0) before (-4,-3)");
  CHECK(dc_motion_before(DcShiftCand{7, 0, 0}, DcShiftCand{7, 0, -1}), "(0,0) wins a tie");
  CHECK(dc_motion_before(DcShiftCand{7, -1, 0}, DcShiftCand{7, 0, 1}), "(-1,0) before (0,1)");

  // 2. score tables: the serial pick, and a fold in an arbitrary order (what a strided scan + butterfly does), equal the first
  //    element of the sorted candidates
  for (int trial = 0; trial < 3000; ++trial) {
    const int S = (int)(rng() % 17), nd = 2 * S + 1, n = nd * nd;
    std::vector<int64_t> sc((size_t)n);
    const int mode = trial % 4;                          // 0: random, 1: two values, 2: constant, 3: extremes
    for (int i = 0; i < n; ++i) {
      if (mode == 0) sc[(size_t)i] = (int64_t)(rng() % 1000000);
      else if (mode == 1) sc[(size_t)i] = (int64_t)(rng() % 2) * 5 + 3;
      else if (mode == 2) sc[(size_t)i] = 42;
      else sc[(size_t)i] = (rng() & 1) ? INT64_MAX : ((rng() & 1) ? INT64_MIN : (int64_t)rng());
    }
    std::vector<DcShiftCand> all;
    for (int i = 0; i < n; ++i) {
      const DcShiftCand c = dc_motion_cand(sc.data(), S, i);
      CHECK(c.score == sc[(size_t)i] && c.dy == i / nd - S && c.dx == i % nd - S && (c.dy + S) * nd + c.dx + S == i, "cand %d", i);
      all.push_back(c);
    }
    std::vector<DcShiftCand> sorted(all);
    std::sort(sorted.begin(), sorted.end(), [](const DcShiftCand a, const DcShiftCand b) { return key(a) < key(b); });
    for (size_t i = 1; i < sorted.size(); ++i) CHECK(key(sorted[i - 1]) < key(sorted[i]), "the order is strict");
    const DcShiftCand serial = dc_motion_pick_serial(sc.data(), S);
    CHECK(key(serial) == key(sorted[0]), "serial pick S=%d trial=%d", S, trial);
    if (mode == 2) CHECK(serial.dy == 0 && serial.dx == 0, "constant scores pick (0,0)");
    // 64 strided partial minima, folded by a butterfly
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
    for (int l = 0; l < 64; ++l) CHECK(key(part[l]) == key(sorted[0]), "butterfly lane %d", l);
  }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("motion_math_check: ok\n");
  return 0;
}
