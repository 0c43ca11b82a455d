// Stand-alone host check of deep_calcium_amd/csrc/series_math.h (the scalar helpers the series-summary kernels are built on),
// meant to be built with -fsanitize=address,undefined and run as a program of its own (tests/test_series_api.py does that):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all series_math_check.cpp -o check && ./check
// The oracles are independent of the code under test: the double -> half rounding is checked against a search over the table
// of all 65536 half values (each decoded exactly by ldexp), the 128-bit helpers against the compiler's __int128.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../deep_calcium_amd/csrc/series_math.h"

static int g_fail = 0;
#define CHECK(cond, ...)                                     \
  do {                                                       \
    if (!(cond)) {                                           \
      if (++g_fail <= 20) { printf("FAIL %s:%d: ", __FILE__, __LINE__); printf(__VA_ARGS__); printf("\n"); } \
    }                                                        \
  } while (0)

static double half_value(unsigned h) {        // finite halves only
  const unsigned ex = (h >> 10) & 0x1f, man = h & 0x3ff;
  const double v = ex == 0 ? ldexp((double)man, -24) : ldexp((double)(man | 0x400), (int)ex - 25);
  return (h & 0x8000) ? -v : v;
}

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rng() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}

// round to nearest even by searching the sorted positive halves; 65520 = the first value that rounds to inf
static uint16_t oracle_f16(double d) {
  static std::vector<double> pos;
  if (pos.empty())
    for (unsigned h = 0; h < 0x7c00; ++h) pos.push_back(half_value(h));      // ascending in h
  if (d != d) return 0x7e00;
  const uint16_t sign = signbit(d) ? 0x8000 : 0;
  const double a = fabs(d);
  if (a >= 65520.0) return sign | 0x7c00;
  const size_t hi = std::upper_bound(pos.begin(), pos.end(), a) - pos.begin();      // pos[hi - 1] <= a < pos[hi]
  const size_t lo = hi - 1;
  if (hi == pos.size()) return sign | (uint16_t)((a - pos[lo] < 65536.0 - a) ? lo : 0x7c00);      // (65504, 65520): the next value up would be 2^16
  const double dl = a - pos[lo], dh = pos[hi] - a;        // both exact: neighbours within a factor of two
  if (dl < dh) return sign | (uint16_t)lo;
  if (dh < dl) return sign | (uint16_t)hi;
  return sign | (uint16_t)((lo & 1) ? hi : lo);
}

static void check_f16() {
  // every half decodes exactly and converts back to itself; NaNs stay NaN, infs stay inf
  for (unsigned h = 0; h < 65536; ++h) {
    const double v = dc_f16_bits_to_f64((uint16_t)h);
    if (((h >> 10) & 0x1f) == 0x1f) {
      if (h & 0x3ff) CHECK(v != v && (dc_f64_to_f16_bits(v) & 0x7c00) == 0x7c00 && (dc_f64_to_f16_bits(v) & 0x3ff), "nan %04x", h);
      else CHECK(isinf(v) && dc_f64_to_f16_bits(v) == h, "inf %04x", h);
      continue;
    }
    CHECK(v == half_value(h) && signbit(v) == (int)((h >> 15) & 1), "decode %04x -> %a", h, v);
    CHECK(dc_f64_to_f16_bits(v) == h, "round trip %04x", h);
  }
  // around every pair of neighbouring halves: the midpoint (a tie) and the doubles next to it on either side, which a
  // conversion through float32 gets wrong (the double next to a tie rounds ONTO the tie in float32)
  for (unsigned h = 0; h < 0x7bff; ++h) {
    const double a = half_value(h), b = half_value(h + 1), mid = 0.5 * (a + b);
    const double probes[] = {mid, nextafter(mid, 0.0), nextafter(mid, 1e9), nextafter(a, 1e9), nextafter(b, 0.0)};
    for (double d : probes)
      for (double s : {1.0, -1.0}) CHECK(dc_f64_to_f16_bits(s * d) == oracle_f16(s * d), "%a near %04x", s * d, h);
  }
  const double edges[] = {0.0, -0.0, 65504.0, 65519.99999999999, 65520.0, 65520.00000000001, 65536.0, 1e300, 5e-324, 2.2250738585072014e-308,
                          ldexp(1.0, -24), ldexp(1.0, -25), nextafter(ldexp(1.0, -25), 1.0), nextafter(ldexp(1.0, -25), 0.0),
                          ldexp(1.0, -26), ldexp(3.0, -25), ldexp(1.0, -14), nextafter(ldexp(1.0, -14), 0.0), ldexp(1.0, -60),
                          ldexp(1.0, -1000), (double)INFINITY};
  for (double d : edges)
    for (double s : {1.0, -1.0}) CHECK(dc_f64_to_f16_bits(s * d) == oracle_f16(s * d), "edge %a", s * d);
  CHECK((dc_f64_to_f16_bits((double)NAN) & 0x7c00) == 0x7c00 && (dc_f64_to_f16_bits((double)NAN) & 0x3ff), "nan");
  for (int i = 0; i < 2000000; ++i) {
    double d;
    if (i & 1) {                                       // random bit patterns with the exponent held near the half range
      const uint64_t b = (rng() & 0x800fffffffffffffull) | ((uint64_t)(1023 - 40 + (int)(rng() % 60)) << 52);
      d = dc_f64_of_bits(b);
    } else {                                           // what the mean chain produces: a half plus x / n
      d = half_value((unsigned)(rng() % 0x7c00)) + (double)((int)(rng() % 98304) - 32768) / (double)(1 + rng() % 5000);
    }
    CHECK(dc_f64_to_f16_bits(d) == oracle_f16(d), "random %a", d);
  }
}

typedef __int128 i128;
static i128 wide(DcI128 a) { return (i128)(((unsigned __int128)(uint64_t)a.hi << 64) | a.lo); }

// nearest double of a 128-bit integer by exact long arithmetic on the magnitude: keep 53 bits, round half to even
static double oracle_to_f64(i128 v) {
  if (v == 0) return 0.0;
  const bool neg = v < 0;
  unsigned __int128 u = neg ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
  int top = 127;
  while (!((u >> top) & 1)) --top;
  double d;
  if (top <= 52) {
    d = (double)(uint64_t)u;
  } else {
    const int sh = top - 52;
    uint64_t q = (uint64_t)(u >> sh);
    const unsigned __int128 rem = u & (((unsigned __int128)1 << sh) - 1), half = (unsigned __int128)1 << (sh - 1);
    if (rem > half || (rem == half && (q & 1))) ++q;
    d = ldexp((double)q, sh);              // q <= 2^53: exact
  }
  return neg ? -d : d;
}

static void check_i128() {
  const int64_t edge[] = {0, 1, -1, 2, -2, INT64_MAX, INT64_MIN, INT64_MIN + 1, 0xffffffffll, 0x100000000ll, -0x100000000ll,
                          2147483647ll, 65535ll * 65535ll * 2147483647ll, -32768ll * 2147483647ll, (1ll << 53) + 1, (1ll << 62)};
  std::vector<int64_t> vals(edge, edge + sizeof(edge) / sizeof(edge[0]));
  for (int i = 0; i < 400; ++i) vals.push_back((int64_t)(rng() >> (rng() % 64)) * ((rng() & 1) ? 1 : -1));
  for (int64_t a : vals)
    for (int64_t b : vals) {
      const DcI128 p = dc_i128_mul(a, b);
      const i128 want = (i128)a * (i128)b;
      CHECK(wide(p) == want, "mul %lld * %lld", (long long)a, (long long)b);
      CHECK(dc_i128_to_f64(p) == oracle_to_f64(want), "to_f64 of %lld * %lld", (long long)a, (long long)b);
      CHECK(wide(dc_i128_neg(p)) == (i128)((unsigned __int128)0 - (unsigned __int128)want), "neg");
      CHECK(dc_i128_is_zero(p) == (want == 0), "is_zero");
    }
  // the numerators as the kernels form them: T * Sxy - Sx * Sy at the extremes of the state
  for (int i = 0; i < 200000; ++i) {
    const int64_t T = 1 + (int64_t)(rng() % 2147483647ull);
    const int64_t sx = (int64_t)(rng() % (uint64_t)(T * 98304)) - T * 32768, sy = (int64_t)(rng() % (uint64_t)(T * 98304)) - T * 32768;
    const int64_t sxy = (int64_t)(rng() % (uint64_t)(T * 4294836225ll));
    const DcI128 n = dc_i128_sub(dc_i128_mul(T, sxy), dc_i128_mul(sx, sy));
    const i128 want = (i128)T * sxy - (i128)sx * sy;
    CHECK(wide(n) == want, "numerator T=%lld", (long long)T);
    CHECK(dc_i128_to_f64(n) == oracle_to_f64(want), "numerator to_f64 T=%lld", (long long)T);
  }
  // ties and sticky bits of the conversion, at every width
  for (int top = 53; top < 127; ++top)
    for (int k = 0; k < 8; ++k) {
      unsigned __int128 u = ((unsigned __int128)1 << top) | ((unsigned __int128)(rng() & ((1ull << 52) - 1)) << (top - 52));
      const int sh = top - 52;
      if (k & 1) u |= (unsigned __int128)1 << (sh - 1);                  // exactly half ...
      if ((k & 2) && sh > 1) u |= 1;                                     // ... plus a sticky bit at the very bottom
      if (k & 4) u |= (unsigned __int128)1 << sh;                        // odd quotient
      for (int s = 0; s < 2; ++s) {
        const i128 v = s ? -(i128)u : (i128)u;
        DcI128 a;
        a.lo = (uint64_t)(unsigned __int128)v;
        a.hi = (int64_t)(uint64_t)((unsigned __int128)v >> 64);
        CHECK(dc_i128_to_f64(a) == oracle_to_f64(v), "tie top=%d k=%d", top, k);
      }
    }
}

int main() {
  check_f16();
  check_i128();
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("series_math_check: ok\n");
  return 0;
}
