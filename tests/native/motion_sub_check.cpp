// Stand-alone host check of the sub-pixel arithmetic of deep_calcium_amd/csrc/motion_math.h (dc_motion_subpixel,
// dc_motion_refine_entry, dc_motion_fine, dc_motion_floor16, dc_motion_frac16, dc_motion_interp), meant to be built with
// -fsanitize=address,undefined and run as a program of its own (tests/test_motion_sub_api.py does that):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all motion_sub_check.cpp -o check && ./check
// The oracle is a brute-force restatement in 128-bit integers: the refinement as the floor division it is defined by, with
// 16 |N| formed in full; the split and the interpolation as floor divisions written out.
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

static const int64_t kTop = (1ll << 62) - 1;             // the largest score

// q as include/dcunet.h defines it, for s0 <= sm and s0 <= sp
static int q_brute(int64_t sm, int64_t s0, int64_t sp) {
  const i128 N = (i128)sm - sp, D = (i128)sm - 2 * (i128)s0 + sp;
  if (D == 0) return 0;
  const i128 a = N < 0 ? -N : N;
  const int m = (int)floor_div(16 * a + D - 1, 2 * D);
  return N < 0 ? -m : m;
}

static void check_q(int64_t sm, int64_t s0, int64_t sp) {
  const int q = dc_motion_subpixel(sm, s0, sp), want = q_brute(sm, s0, sp);
  CHECK(q == want, "q(%lld, %lld, %lld) = %d, not %d", (long long)sm, (long long)s0, (long long)sp, q, want);
  CHECK(q >= -8 && q <= 8, "q in [-8, 8]");
  CHECK(dc_motion_subpixel(sp, s0, sm) == -q, "the mirror image gives the mirrored q");
  if (sm == sp) CHECK(q == 0, "a symmetric neighbourhood gives 0");
  if (sm == s0 && s0 < sp) CHECK(q == -8, "sm == s0 < sp gives exactly -8");
  if (sp == s0 && s0 < sm) CHECK(q == 8, "sp == s0 < sm gives exactly +8");
}

int main() {
  // 1. the refinement of one axis: named cases, every small triple, random triples up to 2^62 - 1
  check_q(0, 0, 0);
  check_q(kTop, 0, kTop);
  check_q(0, 0, kTop);
  check_q(kTop, 0, 0);
  check_q(kTop, kTop, kTop);
  check_q(kTop, kTop - 1, kTop);
  check_q(kTop, 0, kTop - 1);
  check_q(kTop, 1, 2);
  // N and D have the same parity (D - N = 2 (sp - s0)): the tie N / D = 1 / 16 first occurs at N = 2, D = 32
  CHECK(dc_motion_subpixel(9, 0, 8) == 0 && q_brute(9, 0, 8) == 0, "N = 1, D = 17");
  CHECK(dc_motion_subpixel(17, 0, 15) == 0 && dc_motion_subpixel(15, 0, 17) == 0, "the tie at half a sixteenth, N = 2 and D = 32, goes to the pick");
  CHECK(dc_motion_subpixel(19, 0, 13) == 1 && dc_motion_subpixel(13, 0, 19) == -1, "the tie at 1.5 sixteenths, N = 6 and D = 32, goes to the pick's side");
  CHECK(dc_motion_subpixel(11, 1, 8) == 1, "N = 3, D = 17: just beyond a half");
  CHECK(dc_motion_subpixel(8, 0, 8) == 0 && dc_motion_subpixel(0, 0, 5) == -8 && dc_motion_subpixel(5, 0, 0) == 8, "named cases");
  for (int64_t s0 = 0; s0 <= 2; ++s0)
    for (int64_t sm = s0; sm <= s0 + 40; ++sm)
      for (int64_t sp = s0; sp <= s0 + 40; ++sp) check_q(sm, s0, sp);
  for (int trial = 0; trial < 400000; ++trial) {
    const int bits = 1 + (int)(rng() % 62);
    const uint64_t mask = (1ull << bits) - 1;
    int64_t s0 = (int64_t)(rng() & mask), sm = (int64_t)(rng() & mask), sp = (int64_t)(rng() & mask);
    if (trial % 5 == 0) sp = sm + (int64_t)(rng() % 5) - 2;                        // nearly symmetric: small N, large D
    if (trial % 7 == 0) s0 = (sm < sp ? sm : sp) - (int64_t)(rng() % 3);           // nearly flat on one side: |N| close to D
    if (sp < 0) sp = 0;
    if (sp > kTop) sp = kTop;
    const int64_t lo = sm < sp ? sm : sp;
    if (s0 > lo) s0 = lo;
    if (s0 < 0) s0 = 0;
    check_q(sm, s0, sp);
  }
  // scores that are not those of a pick stay defined (no overflow is formed): D <= 0 gives 0
  CHECK(dc_motion_subpixel(0, kTop, 0) == 0 && dc_motion_subpixel(1, 5, 2) == 0, "s0 above its neighbours");
  CHECK(dc_motion_subpixel(INT64_MIN, 0, INT64_MAX) >= -8 && dc_motion_subpixel(INT64_MAX, INT64_MIN, INT64_MAX) <= 8, "wrapping operands");

  // 2. an entry of a table: borders, corners, outside; the table is allocated exactly (the sanitizer sees a read beyond it)
  for (int R = 0; R <= 16; ++R) {
    const int nd = 2 * R + 1;
    std::vector<int64_t> t((size_t)nd * nd);
    for (auto& v : t) v = (int64_t)(rng() % 1000) + 1000;
    for (int py = -R - 2; py <= R + 2; ++py)
      for (int px = -R - 2; px <= R + 2; ++px) {
        const bool inside = py >= -R && py <= R && px >= -R && px <= R;
        int64_t keep = 0;
        if (inside) { keep = t[(size_t)((py + R) * nd + px + R)]; t[(size_t)((py + R) * nd + px + R)] = (int64_t)(rng() % 1000); }
        const DcSubShift q = dc_motion_refine_entry(t.data(), R, py, px);
        int wy = 0, wx = 0;
        if (inside && py > -R && py < R)
          wy = q_brute(t[(size_t)((py + R - 1) * nd + px + R)], t[(size_t)((py + R) * nd + px + R)], t[(size_t)((py + R + 1) * nd + px + R)]);
        if (inside && px > -R && px < R)
          wx = q_brute(t[(size_t)((py + R) * nd + px + R - 1)], t[(size_t)((py + R) * nd + px + R)], t[(size_t)((py + R) * nd + px + R + 1)]);
        CHECK(q.qy == wy && q.qx == wx, "entry R=%d (%d, %d): (%d, %d) != (%d, %d)", R, py, px, q.qy, q.qx, wy, wx);
        if (inside) t[(size_t)((py + R) * nd + px + R)] = keep;
      }
  }
  CHECK(dc_motion_fine(3, -8) == 40 && dc_motion_fine(-16, 8) == -248 && dc_motion_fine(0, 0) == 0, "fine = 16 * whole + q");
  CHECK(dc_motion_fine(2147483647, 0) == -16 && dc_motion_fine(-2147483647 - 1, 5) == 5, "fine wraps, it does not overflow");

  // 3. the split: every small value, the int32 extremes
  const int ev[] = {2147483647, -2147483647 - 1, 2147483632, -2147483632, 2147483633, -2147483633};
  std::vector<int> sv;
  for (int s = -70; s <= 70; ++s) sv.push_back(s);
  for (int s : ev) sv.push_back(s);
  for (int s : sv) {
    const int i = dc_motion_floor16(s), f = dc_motion_frac16(s);
    CHECK((i128)i == floor_div(s, 16) && f >= 0 && f < 16 && (int64_t)16 * i + f == s, "split of %d: (%d, %d)", s, i, f);
  }
  CHECK(dc_motion_floor16(-1) == -1 && dc_motion_frac16(-1) == 15 && dc_motion_floor16(-16) == -1 && dc_motion_frac16(-16) == 0 &&
        dc_motion_floor16(-17) == -2 && dc_motion_frac16(-17) == 15 && dc_motion_floor16(15) == 0, "named splits");

  // 4. the interpolation: every pair of weights at the extremes of int16 and uint16 and at random in between
  const int tv[] = {-32768, -32767, -1, 0, 1, 32767, 32768, 65534, 65535};
  const int ntv = (int)(sizeof(tv) / sizeof(tv[0]));
  for (int fy = 0; fy < 16; ++fy)
    for (int fx = 0; fx < 16; ++fx)
      for (int trial = 0; trial < 600; ++trial) {
        int a[4];
        for (int k = 0; k < 4; ++k) a[k] = trial < 300 ? tv[rng() % (uint64_t)ntv] : (int)(rng() % 98304) - 32768;
        if (trial % 50 == 0) a[1] = a[2] = a[3] = a[0];
        const i128 num = (i128)(16 - fy) * ((16 - fx) * (i128)a[0] + fx * (i128)a[1]) + (i128)fy * ((16 - fx) * (i128)a[2] + fx * (i128)a[3]);
        const int want = (int)floor_div(num + 128, 256), got = dc_motion_interp(a[0], a[1], a[2], a[3], fy, fx);
        CHECK(got == want, "interp (%d %d %d %d) at (%d, %d): %d != %d", a[0], a[1], a[2], a[3], fy, fx, got, want);
        // only the taps with a weight count: the bounds are taken over those
        int lo = a[0], hi = a[0];
        const bool used[4] = {true, fx > 0, fy > 0, fx > 0 && fy > 0};
        for (int k = 1; k < 4; ++k)
          if (used[k]) { lo = a[k] < lo ? a[k] : lo; hi = a[k] > hi ? a[k] : hi; }
        CHECK(got >= lo && got <= hi, "the result lies between the used taps");
        // the kernels interpolate int16 values with the sign bit flipped: adding 32768 to every tap adds it to the result
        if (a[0] < 32768 && a[1] < 32768 && a[2] < 32768 && a[3] < 32768)
          CHECK(dc_motion_interp(a[0] + 32768, a[1] + 32768, a[2] + 32768, a[3] + 32768, fy, fx) == got + 32768, "the flip commutes");
      }
  for (int v : tv) {
    CHECK(dc_motion_interp(v, 12345, -999, 7, 0, 0) == v, "weights (0, 0) return the first tap");
    for (int fy = 0; fy < 16; ++fy)
      for (int fx = 0; fx < 16; ++fx) CHECK(dc_motion_interp(v, v, v, v, fy, fx) == v, "a constant stays constant");
  }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("motion_sub_check: ok\n");
  return 0;
}
