// Stand-alone host check of the temporal-bin rounding in deep_calcium_amd/csrc/series_math.h (dc_series_bin_magic /
// dc_series_bin_round: floor((2 s + b) / (2 b)) by a multiplication), meant to be built with -fsanitize=address,undefined and run
// as a program of its own (tests/test_tbin_api.py does that):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all series_bin_check.cpp -o check && ./check
// The oracle is 64-bit floor division.  Every b in [1, 64]: the extremes of both 16-bit types (b frames at -32768, 32767, 65535),
// every sum around every half -- s = k b + floor(b / 2) + d for every mean k in [-32768, 65535] and d in [-2, 2] --, a window
// around 0, a coarse sweep of the whole range, and the promise that the result lies between the smallest and the largest frame.
#include <stdint.h>
#include <stdio.h>

#include "../../deep_calcium_amd/csrc/series_math.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                     \
  do {                                                       \
    if (!(cond)) {                                           \
      if (++g_fail <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
    }                                                        \
  } while (0)

static int64_t floor_div(int64_t n, int64_t d) {        // d > 0
  int64_t q = n / d;
  if (n % d < 0) --q;
  return q;
}

static long g_checked = 0;
static void check(int64_t s, int b, uint32_t magic) {
  if (s < -32768ll * b || s > 65535ll * b) return;       // no sum of b 16-bit values
  const int64_t want = floor_div(2 * s + b, 2ll * b);
  const int got = dc_series_bin_round((int)s, b, magic);
  CHECK(got == want, "b = %d, s = %lld: %d, floor division gives %lld", b, (long long)s, got, (long long)want);
  ++g_checked;
}

int main() {
  for (int b = 1; b <= 64; ++b) {
    const uint32_t magic = dc_series_bin_magic(b);
    CHECK((uint64_t)magic == 0x100000000ull / (uint64_t)(2 * b) + 1, "b = %d: magic %u", b, magic);
    // the extremes: b equal frames give that frame
    const int64_t ext[3] = {-32768, 32767, 65535};
    for (int e = 0; e < 3; ++e) {
      CHECK(dc_series_bin_round((int)(ext[e] * b), b, magic) == ext[e], "b = %d: %lld frames of %lld", b, (long long)b, (long long)ext[e]);
      for (int d = -3 * b; d <= 3 * b; ++d) check(ext[e] * b + d, b, magic);
    }
    // around every half
    for (int64_t k = -32768; k <= 65535; ++k)
      for (int d = -2; d <= 2; ++d) check(k * b + b / 2 + d, b, magic);
    // around zero, where the floor and the truncation part ways
    for (int64_t s = -4 * b - 4; s <= 4 * b + 4; ++s) check(s, b, magic);
    // a coarse sweep of the whole range
    for (int64_t s = -32768ll * b; s <= 65535ll * b; s += 7) check(s, b, magic);
  }
  // (-1, -2) -> -1: the mean -1.5 rounds half UP; 64 frames of the extremes stay what they are
  CHECK(dc_series_bin_round(-3, 2, dc_series_bin_magic(2)) == -1, "(-1, -2)");
  CHECK(dc_series_bin_round(-32768 * 64, 64, dc_series_bin_magic(64)) == -32768, "-32768 * 64");
  CHECK(dc_series_bin_round(65535 * 64, 64, dc_series_bin_magic(64)) == 65535, "65535 * 64");
  // between the smallest and the largest frame of the bin: two values lo <= hi, i of them hi
  for (int b = 2; b <= 64; b += 31)
    for (int lo = -32768; lo <= 65535; lo += 4099)
      for (int hi = lo; hi <= 65535 && (lo >= 0 || hi <= 32767); hi += 1021)
        for (int i = 0; i <= b; ++i) {
          const int r = dc_series_bin_round(lo * (b - i) + hi * i, b, dc_series_bin_magic(b));
          CHECK(lo <= r && r <= hi, "b = %d: %d of %d and %d of %d give %d", b, b - i, lo, i, hi, r);
        }
  if (g_fail) {
    printf("series_bin_check: %d failures\n", g_fail);
    return 1;
  }
  printf("series_bin_check: ok (%ld sums)\n", g_checked);
  return 0;
}
