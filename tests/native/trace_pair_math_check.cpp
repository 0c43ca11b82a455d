// Stand-alone host check of deep_calcium_amd/csrc/trace_pair_math.h (the scalar arithmetic of the ROI trace-pair correlation),
// meant to be built with -fsanitize=address,undefined and run as a program of its own (tests/test_merge_api.py does that):
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all trace_pair_math_check.cpp -o check && ./check
// The oracle is the compiler's __int128 (signed: an overflow of the oracle itself would be reported by the sanitizer).  Three
// things: the segment plan against the words of series.detrend_plan; the per-segment term and the pooled numerators against
// __int128 with both rows AT THE BOUND +-floor(2^62 / max(M, T)), where the products need 112 bits and the numerators 124; and
// the range predicate at its edges.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../deep_calcium_amd/csrc/trace_pair_math.h"

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
static DcI128 narrow(i128 v) { DcI128 r; r.lo = (uint64_t)(u128)v; r.hi = (int64_t)(v >> 64); return r; }
static i128 iabs(i128 v) { return v < 0 ? -v : v; }
static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// the plan by the words of series.detrend_plan: n = max(1, T // L) segments, n - 1 of L frames and a last one of T - (n - 1) L;
// mult = M / len with M = L * L_last (M = T when n == 1)
static void check_plan(int64_t T, int64_t L) {
  const DcTracePairPlan p = dc_trace_pair_plan(T, L);
  const int64_t n = L > 0 && T / L > 1 ? T / L : 1;
  const int64_t last = n == 1 ? T : T - (n - 1) * L, M = n == 1 ? T : L * last;
  CHECK(p.n == n && p.last == last && p.M == M, "plan(T = %lld, L = %lld): n %lld last %lld M %lld", (long long)T, (long long)L, (long long)p.n,
        (long long)p.last, (long long)p.M);
  if (n > 1) CHECK(last >= L && last < 2 * L, "L_last = %lld of L = %lld", (long long)last, (long long)L);
  // every segment of a short plan; of a long one the first ones, the middle and the last ones (every full segment has one shape)
  int64_t at = 0, end = 0;
  for (int64_t s = 0; s < p.n; s = (p.n <= 4096 || s < 2 || s >= p.n - 3) ? s + 1 : (s < p.n / 2 ? p.n / 2 : p.n - 3)) {
    int64_t start, len, mult;
    dc_trace_pair_segment(p, s, &start, &len, &mult);
    const int64_t want_len = n == 1 ? T : (s < n - 1 ? L : last);
    if (p.n > 4096) at = s * L;                      // where the segments before it end, by the words of the plan
    CHECK(start == at && len == want_len && len * mult == M, "segment %lld of plan(T = %lld, L = %lld): start %lld len %lld mult %lld", (long long)s,
          (long long)T, (long long)L, (long long)start, (long long)len, (long long)mult);
    if (len > 0) CHECK(mult == M / len && dc_detrend_segment_ok(len, mult), "mult of segment %lld", (long long)s);
    at += len;
    end = start + len;
  }
  CHECK(end == T, "the segments of plan(T = %lld, L = %lld) end at %lld", (long long)T, (long long)L, (long long)end);
  // L > T / 2 is one segment: the plan of seg_len = 0
  if (L > 0 && 2 * L > T) {
    const DcTracePairPlan z = dc_trace_pair_plan(T, 0);
    CHECK(p.n == 1 && z.n == 1 && p.L == z.L && p.last == z.last && p.M == z.M, "L = %lld > T / 2 = %lld / 2 is not the plan of 0", (long long)L, (long long)T);
  }
}

// A segment in which the two rows take two value pairs: (x0, y0) for k frames, (x1, y1) for the other len - k.
struct Seg { int64_t len, mult, k, x0, y0, x1, y1; };

static void add_segment(const Seg& s, DcI128 got[3], i128 want[3], i128* worst_product) {
  const i128 k = s.k, m = s.len - s.k;
  const i128 ax = k * s.x0 + m * s.x1, ay = k * s.y0 + m * s.y1;
  const i128 gxx = k * s.x0 * s.x0 + m * s.x1 * s.x1, gxy = k * s.x0 * s.y0 + m * s.x1 * s.y1, gyy = k * s.y0 * s.y0 + m * s.y1 * s.y1;
  CHECK(iabs(ax) <= ((i128)1 << 62) && iabs(ay) <= ((i128)1 << 62), "a segment's sum leaves 2^62");
  const i128 t[3] = {(i128)s.mult * ((i128)s.len * gxx - ax * ax), (i128)s.mult * ((i128)s.len * gxy - ax * ay),
                     (i128)s.mult * ((i128)s.len * gyy - ay * ay)};
  const DcI128 d[3] = {dc_trace_pair_term(s.len, s.mult, narrow(gxx), (int64_t)ax, (int64_t)ax),
                       dc_trace_pair_term(s.len, s.mult, narrow(gxy), (int64_t)ax, (int64_t)ay),
                       dc_trace_pair_term(s.len, s.mult, narrow(gyy), (int64_t)ay, (int64_t)ay)};
  for (int q = 0; q < 3; ++q) {
    CHECK(wide(d[q]) == t[q], "term %d of a segment of %lld frames, mult %lld", q, (long long)s.len, (long long)s.mult);
    got[q] = dc_i128_add(got[q], d[q]);
    want[q] += t[q];
  }
  CHECK(t[0] >= 0 && t[2] >= 0, "a segment's N(x, x) is negative");
  const i128 prod = (i128)s.mult * s.len * gxx;      // the largest product dc_detrend_term_wide forms before it subtracts
  if (prod > *worst_product) *worst_product = prod;
  // the single products of the kernel's accumulation: dc_i128_mul at the bound
  CHECK(wide(dc_i128_mul(s.x0, s.y0)) == (i128)s.x0 * s.y0 && wide(dc_i128_mul(s.x1, s.y1)) == (i128)s.x1 * s.y1, "x * y at the bound");
}

// uniform in [-B, B], B <= 2^62: the span 2 B + 1 and the draw are formed in uint64
static int64_t pick(int64_t B) { return (int64_t)(rng() % (2 * (uint64_t)B + 1) - (uint64_t)B); }

// both rows at +-B, B = floor(2^62 / max(M, T)), over the whole plan; mode 0: y == x (the diagonal), 1: y == -x, 2: y alternates by
// segment, 3: random values within the bound
static void check_bound(int64_t T, int64_t L, int mode) {
  const DcTracePairPlan p = dc_trace_pair_plan(T, L);
  const int64_t big = p.M > T ? p.M : T, B = DC_TRACE_PAIR_RANGE / big;
  CHECK(dc_trace_pair_range_ok(B, p, T) && dc_trace_pair_range_ok(-B, p, T) && !dc_trace_pair_range_ok(B + 1, p, T) &&
        !dc_trace_pair_range_ok(-B - 1, p, T), "the bound of plan(T = %lld, L = %lld) is not %lld", (long long)T, (long long)L, (long long)B);
  DcI128 got[3] = {{0, 0}, {0, 0}, {0, 0}};
  i128 want[3] = {0, 0, 0}, worst = 0;
  // at most 4096 segments are walked: beyond that the plan's first, middle and last ones (every full segment is the same shape)
  const int64_t step = p.n > 4096 ? p.n / 2048 : 1;
  int64_t walked = 0;
  for (int64_t s = 0; s < p.n; s = (s == p.n - 1 || s + step < p.n - 1) ? s + step : p.n - 1) {
    Seg g;
    int64_t start;
    dc_trace_pair_segment(p, s, &start, &g.len, &g.mult);
    g.k = mode == 3 ? (int64_t)(rng() % (uint64_t)(g.len + 1)) : g.len / 2;
    g.x0 = mode == 3 ? pick(B) : B;
    g.x1 = mode == 3 ? pick(B) : -B;
    g.y0 = mode == 0 ? g.x0 : mode == 1 ? -g.x0 : mode == 2 ? ((s & 1) ? -B : B) : pick(B);
    g.y1 = mode == 0 ? g.x1 : mode == 1 ? -g.x1 : mode == 2 ? ((s & 1) ? B : -B) : pick(B);
    add_segment(g, got, want, &worst);
    ++walked;
  }
  for (int q = 0; q < 3; ++q) CHECK(wide(got[q]) == want[q], "pooled numerator %d, plan(T = %lld, L = %lld), mode %d", q, (long long)T, (long long)L, mode);
  const i128 lim = (i128)1 << 124;
  CHECK(want[0] >= 0 && want[0] <= lim && want[2] >= 0 && want[2] <= lim && iabs(want[1]) <= lim && worst <= lim,
        "magnitudes, plan(T = %lld, L = %lld), mode %d", (long long)T, (long long)L, mode);
  // two levels, half and half: a segment's term is mult (len^2 - (k - m)^2) B^2 >= (8 / 9) M len B^2, so N(x, x) reaches at least half
  // of the bound M T B^2 -- and with one segment (M = T) that is 2^123: the high words are in use
  if (mode < 3 && walked == p.n && T > 1) {
    CHECK(want[0] * 2 >= (i128)p.M * T * B * B, "mode %d at T = %lld, L = %lld: N(x, x) = %g is below half its bound", mode, (long long)T, (long long)L,
          (double)want[0]);
    if (p.n == 1) CHECK(want[0] > ((i128)1 << 122), "mode %d at T = %lld does not reach 2^122: %g", mode, (long long)T, (double)want[0]);
  }
  const DcFpNum n = {got[0], got[1], got[2]}, sw = {got[2], got[1], got[0]};
  const float r = dc_fp_corr(n);
  CHECK(r >= -1.f && r <= 1.f && bits(r) == bits(dc_fp_corr(sw)), "corr %.9g: range or symmetry", (double)r);
  if (mode == 0 && T > 1) CHECK(r == 1.f, "the diagonal gives %.9g", (double)r);
  if (mode == 1 && T > 1) CHECK(r == -1.f, "the mirror image gives %.9g", (double)r);
}

int main() {
  CHECK(DC_TRACE_PAIR_RANGE == ((int64_t)1 << 62) && DC_TRACE_PAIR_MAX_PAIRS == (1L << 24), "the limits");

  // ---- the plan ------------------------------------------------------------------------------------------------------------------
  {
    const int64_t Ts[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 255, 256, 257, 1000, 1024, 4095, 4096, 8191, 8192, 8193, 12287, 100000, DC_FP_MAX_FRAMES};
    const int64_t Ls[] = {0, 2, 3, 64, 100, 128, 4095, 4096};
    for (int64_t T : Ts)
      for (int64_t L : Ls) check_plan(T, L);
    for (int i = 0; i < 20000; ++i) check_plan((int64_t)(rng() % (uint64_t)DC_FP_MAX_FRAMES >> (rng() % 31)), 2 + (int64_t)(rng() % 4095));
    // the words of the issue: T = 1000, L = 128 is 6 x 128 and one of 232; T = 5, L = 2 is 2 + 3
    DcTracePairPlan p = dc_trace_pair_plan(1000, 128);
    CHECK(p.n == 7 && p.last == 232 && p.M == 128 * 232, "T = 1000, L = 128");
    p = dc_trace_pair_plan(5, 2);
    CHECK(p.n == 2 && p.last == 3 && p.M == 6, "T = 5, L = 2");
  }

  // ---- the terms and the pooled numerators at the bound ----------------------------------------------------------------------------
  for (int mode = 0; mode < 4; ++mode) {
    check_bound(1, 0, mode);
    check_bound(2, 0, mode);
    check_bound(5, 2, mode);
    check_bound(257, 2, mode);
    check_bound(1000, 0, mode);
    check_bound(1000, 128, mode);
    check_bound(8192, 128, mode);
    check_bound(12287, 4096, mode);                  // 2 segments, the longest last one: M = 4096 * 8191 > T
    check_bound(DC_FP_MAX_FRAMES, 0, mode);          // one segment of 2^31 - 1 frames
    check_bound(DC_FP_MAX_FRAMES, 4096, mode);       // the most segments of the longest kind
    check_bound(DC_FP_MAX_FRAMES, 2, mode);
  }
  // ROI sums inside the volume limits lie inside the range: |S| <= 65535 A with max(M, T) A <= 2^46
  {
    const DcTracePairPlan p = dc_trace_pair_plan(12287, 4096);
    const int64_t A = DC_DETREND_MAX_VOLUME / p.M;
    CHECK(dc_trace_pair_range_ok(65535 * A, p, 12287) && dc_trace_pair_range_ok(-65536 * A, p, 12287), "ROI sums of the largest area");
  }

  // ---- the range predicate ------------------------------------------------------------------------------------------------------
  {
    const DcTracePairPlan one = dc_trace_pair_plan(1, 0), none = dc_trace_pair_plan(0, 0);
    CHECK(dc_trace_pair_range_ok(DC_TRACE_PAIR_RANGE, one, 1) && !dc_trace_pair_range_ok(DC_TRACE_PAIR_RANGE + 1, one, 1), "T = 1");
    CHECK(dc_trace_pair_range_ok(-DC_TRACE_PAIR_RANGE, one, 1) && !dc_trace_pair_range_ok(INT64_MIN, one, 1) && !dc_trace_pair_range_ok(INT64_MAX, one, 1),
          "the ends of int64");
    CHECK(dc_trace_pair_range_ok(INT64_MIN, none, 0) && dc_trace_pair_range_ok(0, one, 1), "nothing is read of an empty row");
    const DcTracePairPlan p = dc_trace_pair_plan(1000, 128);      // M = 29696 > T
    CHECK(dc_trace_pair_range_ok(DC_TRACE_PAIR_RANGE / 29696, p, 1000) && !dc_trace_pair_range_ok(DC_TRACE_PAIR_RANGE / 29696 + 1, p, 1000), "M > T decides");
    const DcTracePairPlan q = dc_trace_pair_plan(1000, 2);        // M = 4 < T
    CHECK(dc_trace_pair_range_ok(DC_TRACE_PAIR_RANGE / 1000, q, 1000) && !dc_trace_pair_range_ok(DC_TRACE_PAIR_RANGE / 1000 + 1, q, 1000), "T > M decides");
  }
  if (g_fail) { printf("%d checks failed\n", g_fail); return 1; }
  printf("trace_pair_math_check: ok\n");
  return 0;
}
