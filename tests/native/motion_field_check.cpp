// Stand-alone host check of the block geometry and the shift field of deep_calcium_amd/csrc/motion_math.h (dc_block_edge,
// dc_block_axis_ok, dc_field_tap_edges, dc_field_blend, dc_field_value, dc_field_from_rows, dc_field_from_delta, dc_motion_clamp), meant to be
// built with -fsanitize=address,undefined and run as a program of its own (tests/test_motion_block_api.py does that):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all motion_field_check.cpp -o check && ./check
// The oracle is a brute-force restatement in 128-bit integers: edges by a search for the largest e with e * B <= i * n, taps by a
// scan over all centres, the field by a floor division written out.
#include <stdio.h>
#include <stdlib.h>

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

typedef __int128 i128;

static i128 floor_div(i128 a, i128 b) {                  // b > 0
  i128 q = a / b;
  if (a % b != 0 && a < 0) --q;
  return q;
}

// e(i) = floor(i * n / B) without the division: the largest e with e * B <= i * n, found by bisection
static int edge_brute(int i, int n, int B) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) / 2;
    if ((i128)mid * B <= (i128)i * n) lo = mid; else hi = mid - 1;
  }
  return (int)lo;
}

static void check_axis(int n, int B, bool every_pixel) {
  std::vector<int64_t> e((size_t)B + 1), c2((size_t)B);
  std::vector<int> e32((size_t)B + 1);                   // the table dc_field_tap_edges reads: exactly B + 1 entries
  for (int i = 0; i <= B; ++i) {
    e[(size_t)i] = edge_brute(i, n, B);
    e32[(size_t)i] = (int)e[(size_t)i];
    CHECK(dc_block_edge(i, n, B) == e[(size_t)i], "edge i=%d n=%d B=%d", i, n, B);
  }
  CHECK(e[0] == 0 && e[(size_t)B] == n, "the edges span the axis n=%d B=%d", n, B);
  for (int i = 0; i < B; ++i) {
    c2[(size_t)i] = e[(size_t)i] + e[(size_t)i + 1] - 1;
    if (i) CHECK(c2[(size_t)i] > c2[(size_t)i - 1], "the centres increase strictly n=%d B=%d", n, B);
  }
  // the margins M at which every clipped block keeps a pixel, by looking at every block
  for (int M = 0; M <= 24 && M <= n; ++M) {
    bool want = true;
    for (int i = 0; i < B; ++i) {
      const int64_t lo = e[(size_t)i] > M ? e[(size_t)i] : M, hi = e[(size_t)i + 1] < n - M ? e[(size_t)i + 1] : n - M;
      if (lo >= hi) want = false;
    }
    CHECK(dc_block_axis_ok(n, B, M) == want, "axis_ok n=%d B=%d M=%d", n, B, M);
  }
  const int step = every_pixel ? 1 : (n / 997 + 1);
  for (int64_t yy = 0; yy < n; yy += step) {
    // the last pixels of a sparse walk are visited as well
    const int y = (!every_pixel && yy + step >= n) ? n - 1 : (int)yy;
    const int64_t p = 2 * (int64_t)y;
    int i0, i1, w;
    if (B == 1 || p <= c2[0]) {
      i0 = i1 = w = 0;
    } else if (p >= c2[(size_t)B - 1]) {
      i0 = i1 = B - 1;
      w = 0;
    } else {
      i0 = 0;
      for (int i = 0; i < B; ++i)
        if (c2[(size_t)i] <= p) i0 = i;
      i1 = i0 + 1;
      w = (int)floor_div((i128)256 * (p - c2[(size_t)i0]), c2[(size_t)i1] - c2[(size_t)i0]);
    }
    const DcFieldTap t = dc_field_tap_edges(y, e32.data(), B);
    CHECK(t.i0 == i0 && t.i1 == i1 && t.w == w, "tap y=%d n=%d B=%d: (%d %d %d) != (%d %d %d)", y, n, B, t.i0, t.i1, t.w, i0, i1, w);
    CHECK(t.i0 >= 0 && t.i1 < B && t.w >= 0 && t.w < 256 && (t.w == 0 || t.i1 == t.i0 + 1), "tap range y=%d n=%d B=%d", y, n, B);
  }
}

int main() {
  // 1. geometry and taps: every pixel of small axes for every B, a sparse walk of the largest ones
  for (int B = 1; B <= 32; ++B)
    for (int n = B; n <= 140; ++n) check_axis(n, B, true);
  const int big[] = {512, 1000, 1100, 65535, 65536, 1 << 20, (1 << 30) - 1, 1 << 30};
  const int bs[] = {1, 2, 3, 7, 31, 32};
  for (int n : big)
    for (int B : bs) check_axis(n, B, n <= 1100);
  for (int trial = 0; trial < 300; ++trial) {
    const int B = 1 + (int)(rng() % 32);
    const int n = B + (int)(rng() % ((1u << 30) - 32));
    check_axis(n, B, false);
  }

  // 2. the field: against 128-bit arithmetic, at the int32 extremes, for every pair of weights on a grid and at random
  const int64_t sv[] = {0, 1, -1, 7, -8, 2147483647ll, -2147483648ll, 2147483646ll, -2147483647ll, 65536, -65536, 32768, -32767};
  const int nsv = (int)(sizeof(sv) / sizeof(sv[0]));
  long n_small = 0;
  for (int trial = 0; trial < 400000; ++trial) {
    int64_t s[4];
    for (int k = 0; k < 4; ++k) s[k] = (trial % 3 == 0) ? (int64_t)(int32_t)rng() : sv[rng() % (uint64_t)nsv];
    if (trial % 4 == 1) {                                // neighbours a few pixels apart around any base: the small-difference path,
      const int64_t base = s[0];                         // up to and beyond its limit of 2^14 pixels
      const int64_t reach = (trial % 8 == 1) ? 20 : 16400;
      for (int k = 0; k < 4; ++k) {
        s[k] = base + (int64_t)(rng() % (uint64_t)(2 * reach + 1)) - reach;
        s[k] = s[k] > 2147483647ll ? 2147483647ll : (s[k] < -2147483648ll ? -2147483648ll : s[k]);
      }
    }
    const int w = (trial % 5 == 0) ? (int)(rng() % 2) * 255 : (int)(rng() % 256), v = (trial % 7 == 0) ? 0 : (int)(rng() % 256);
    const i128 num = (i128)(256 - w) * ((i128)(256 - v) * s[0] + (i128)v * s[1]) + (i128)w * ((i128)(256 - v) * s[2] + (i128)v * s[3]);
    const int64_t want = (int64_t)floor_div(num + 32768, 65536);
    const int64_t got = dc_field_value(s[0], s[1], s[2], s[3], w, v);
    CHECK(got == want, "field trial %d", trial);
    const int64_t rows = dc_field_from_rows(dc_field_blend(s[0], s[2], w), dc_field_blend(s[1], s[3], w), v);
    CHECK(rows == want, "field from the row blends, trial %d", trial);
    const int64_t a0 = dc_field_blend(s[0], s[2], w), d = dc_field_blend(s[1], s[3], w) - a0;
    if (dc_field_delta_small(d)) {
      ++n_small;
      CHECK(dc_field_from_delta(a0, (int)d, v) == want, "field from the difference, trial %d", trial);
    }
    int64_t lo = s[0], hi = s[0];
    for (int k = 1; k < 4; ++k) { lo = s[k] < lo ? s[k] : lo; hi = s[k] > hi ? s[k] : hi; }
    CHECK(got >= lo && got <= hi, "the field stays in the hull, trial %d", trial);
    if (s[0] == s[1] && s[1] == s[2] && s[2] == s[3]) CHECK(got == s[0], "equal shifts, trial %d", trial);
  }
  CHECK(n_small > 100000, "the small-difference path was exercised: %ld", n_small);
  CHECK(dc_field_delta_small((1 << 22) - 1) && !dc_field_delta_small(1 << 22) && dc_field_delta_small(1 - (1 << 22)) && !dc_field_delta_small(-(1 << 22)),
        "the limit of the small difference");
  for (int64_t s : sv)
    for (int w = 0; w < 256; w += 15)
      for (int v = 0; v < 256; v += 17) CHECK(dc_field_value(s, s, s, s, w, v) == s, "a uniform field is that shift");
  CHECK(dc_field_value(2147483647ll, -2147483648ll, 2147483647ll, -2147483648ll, 0, 128) == 0, "half way between the extremes");
  CHECK(dc_floor_div_65536(-1) == -1 && dc_floor_div_65536(-65536) == -1 && dc_floor_div_65536(-65537) == -2 && dc_floor_div_65536(65535) == 0,
        "floor division");

  // 3. the clamp
  const int cv[] = {0, 1, -1, 16, -16, 17, -17, 1000, -1000, 2147483647, -2147483647 - 1};
  for (int S = 0; S <= 16; ++S)
    for (int v : cv) {
      const int c = dc_motion_clamp(v, S);
      CHECK(c >= -S && c <= S && (v < -S || v > S || c == v), "clamp %d to %d", v, S);
    }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("motion_field_check: ok\n");
  return 0;
}
