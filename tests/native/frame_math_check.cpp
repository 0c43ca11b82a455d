// Stand-alone host check of deep_calcium_amd/csrc/frame_math.h (the scalar arithmetic of the per-frame quality scores), meant to
// be built with -fsanitize=address,undefined and run as a program of its own (tests/test_frames_api.py does that):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all frame_math_check.cpp -o check && ./check
// The oracle is the compiler's __int128 (signed: an overflow of the oracle itself would be reported by the sanitizer).  Three
// things: the numerators against __int128 AT THE BOUNDS -- every pixel 65535 or -32768 over n = 2^28 pixels, where a reaches 2^44
// and b and c 2^60 --, and on random moments inside them; the exact cases of the correlation (1, -1, 0); the rectangle and the mean.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../deep_calcium_amd/csrc/frame_math.h"

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

static i128 wide(DcI128 a) { return (i128)(((u128)(uint64_t)a.hi << 64) | a.lo); }
static i128 iabs(i128 v) { return v < 0 ? -v : v; }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static void check_numerators(int64_t n, int64_t a, int64_t b, int64_t c, int64_t ta, int64_t tb, const char* what) {
  const DcFpNum got = dc_frame_numerators(n, a, b, c, ta, tb);
  const i128 nxx = (i128)n * b - (i128)a * a, nxt = (i128)n * c - (i128)a * ta, ntt = (i128)n * tb - (i128)ta * ta;
  CHECK(wide(got.cxx) == nxx && wide(got.cxl) == nxt && wide(got.cll) == ntt, "numerators (%s): n %lld a %lld b %lld c %lld ta %lld tb %lld", what,
        (long long)n, (long long)a, (long long)b, (long long)c, (long long)ta, (long long)tb);
  const i128 lim = (i128)1 << 89;
  CHECK(iabs(nxx) < lim && iabs(nxt) < lim && iabs(ntt) < lim, "a numerator leaves 2^89 (%s)", what);
}

// the moments of a frame of p pixels at value x and n - p at value y, against a template of q pixels at u (the FIRST q) and the rest at v
static void moments_of(int64_t n, int64_t p, int64_t x, int64_t y, int64_t q, int64_t u, int64_t v, int64_t* a, int64_t* b, int64_t* c, int64_t* ta,
                       int64_t* tb) {
  *a = p * x + (n - p) * y;
  *b = p * x * x + (n - p) * y * y;
  *ta = q * u + (n - q) * v;
  *tb = q * u * u + (n - q) * v * v;
  const int64_t lo = p < q ? p : q, hi = p < q ? q : p;         // [0, lo): x u; [lo, hi): x v or y u; [hi, n): y v
  *c = lo * x * u + (hi - lo) * (p < q ? y * u : x * v) + (n - hi) * y * v;
}

int main() {
  const int64_t N = DC_FRAME_MAX_PIXELS;
  CHECK(N == ((int64_t)1 << 28), "DC_FRAME_MAX_PIXELS");
  // ---- at the bounds: every pixel an extreme of its type, n = 2^28 ----
  const int64_t ext[4] = {65535, -32768, 0, 32767};
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j)
      for (int k = 0; k < 4; ++k)
        for (int l = 0; l < 4; ++l) {
          const int64_t splits[5] = {0, 1, N / 2, N - 1, N};
          for (int s = 0; s < 5; ++s)
            for (int t = 0; t < 5; ++t) {
              int64_t a, b, c, ta, tb;
              moments_of(N, splits[s], ext[i], ext[j], splits[t], ext[k], ext[l], &a, &b, &c, &ta, &tb);
              CHECK(llabs(a) < ((int64_t)1 << 44) && b < ((int64_t)1 << 60) && llabs(c) < ((int64_t)1 << 60), "the moments leave their range");
              check_numerators(N, a, b, c, ta, tb, "bounds");
            }
        }
  {
    int64_t a, b, c, ta, tb;
    moments_of(N, N, 65535, 0, N, 65535, 0, &a, &b, &c, &ta, &tb);
    CHECK(a == N * 65535 && b == N * 65535 * 65535 && c == b && ta == a && tb == b, "all 65535");
    const DcFpNum z = dc_frame_numerators(N, a, b, c, ta, tb);
    CHECK(dc_i128_is_zero(z.cxx) && dc_i128_is_zero(z.cxl) && dc_i128_is_zero(z.cll) && bits(dc_fp_corr(z)) == bits(0.f), "a constant frame: zeros, corr 0");
    CHECK(bits(dc_frame_mean(a, N)) == bits(65535.f), "mean of all 65535");
    moments_of(N, N, -32768, 0, N, -32768, 0, &a, &b, &c, &ta, &tb);
    CHECK(a == -N * 32768 && b == N * 32768 * 32768 && bits(dc_frame_mean(a, N)) == bits(-32768.f), "all -32768");
  }
  // ---- random moments of two-valued frames: any n, any split ----
  for (int it = 0; it < 200000; ++it) {
    const int64_t n = 1 + (int64_t)(rng() % (uint64_t)N);
    const int64_t p = (int64_t)(rng() % (uint64_t)(n + 1)), q = (int64_t)(rng() % (uint64_t)(n + 1));
    const bool uns = rng() & 1;
    int64_t val[4];
    for (int k = 0; k < 4; ++k) val[k] = uns ? (int64_t)(rng() % 65536) : (int64_t)(rng() % 65536) - 32768;
    int64_t a, b, c, ta, tb;
    moments_of(n, p, val[0], val[1], q, val[2], val[3], &a, &b, &c, &ta, &tb);
    check_numerators(n, a, b, c, ta, tb, "random");
    const DcFpNum num = dc_frame_numerators(n, a, b, c, ta, tb);
    const float r = dc_fp_corr(num);
    CHECK(r >= -1.f && r <= 1.f, "corr %g outside [-1, 1]", (double)r);
    const double exact_mean = (double)((long double)a / (long double)n);
    CHECK(fabs((double)dc_frame_mean(a, n) - exact_mean) <= fabs(exact_mean) * 6.0e-8 + 1e-30, "mean");
    // frame == template: exactly 1 where it varies, exactly 0 where it does not
    const DcFpNum same = dc_frame_numerators(n, a, b, b, a, b);
    const bool varies = wide(same.cxx) > 0;
    CHECK(bits(dc_fp_corr(same)) == bits(varies ? 1.f : 0.f), "frame == template: %g", (double)dc_fp_corr(same));
    // frame = k - template, k = 7: a' = 7 n - a, b' = 49 n - 14 a + b, c' = 7 a - b (against the template a, b): exactly -1
    const int64_t k = 7;
    const DcFpNum mirror = dc_frame_numerators(n, k * n - a, k * k * n - 2 * k * a + b, k * a - b, a, b);
    CHECK(bits(dc_fp_corr(mirror)) == bits(varies ? -1.f : 0.f), "frame = k - template: %g", (double)dc_fp_corr(mirror));
  }
  // n == 1: nothing varies
  CHECK(bits(dc_fp_corr(dc_frame_numerators(1, -5, 25, 15, -3, 9))) == bits(0.f), "n == 1");
  // ---- the rectangle ----
  CHECK(dc_frame_rect_pixels(5, 7, 0, 5, 0, 7) == 35 && dc_frame_rect_pixels(5, 7, 4, 5, 6, 7) == 1, "rect inside");
  CHECK(dc_frame_rect_pixels(5, 7, 0, 6, 0, 7) == -1 && dc_frame_rect_pixels(5, 7, 0, 5, 0, 8) == -1 && dc_frame_rect_pixels(5, 7, -1, 5, 0, 7) == -1 &&
            dc_frame_rect_pixels(5, 7, 0, 5, -1, 7) == -1, "rect outside");
  CHECK(dc_frame_rect_pixels(5, 7, 2, 2, 0, 7) == -1 && dc_frame_rect_pixels(5, 7, 0, 5, 3, 3) == -1 && dc_frame_rect_pixels(5, 7, 3, 2, 0, 7) == -1, "rect empty");
  CHECK(dc_frame_rect_pixels(32768, 32768, 0, 32768, 0, 32768) == ((int64_t)1 << 30), "rect of 2^30 pixels");
  if (g_fail) {
    printf("frame_math_check: %d FAILED\n", g_fail);
    return 1;
  }
  printf("frame_math_check: ok\n");
  return 0;
}
