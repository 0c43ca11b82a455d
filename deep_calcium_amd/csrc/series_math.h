// Exact scalar helpers of the series-summary and ROI-trace kernels (series.hip, traces.hip): binary16 <-> binary64 conversion with ONE rounding, and the
// 128-bit integers the correlation / variance numerators are formed in.  Plain C++ on purpose -- no HIP header, no intrinsic beyond
// __builtin_clzll -- so the same inline functions compile for the device and into a stand-alone host program
// (tests/native/series_math_check.cpp, run under the address / undefined-behaviour sanitizers).
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DC_HD __host__ __device__ inline
#else
#define DC_HD inline
#endif

DC_HD uint64_t dc_bits_of_f64(double d) { uint64_t u; memcpy(&u, &d, 8); return u; }
DC_HD double dc_f64_of_bits(uint64_t u) { double d; memcpy(&d, &u, 8); return d; }

// binary64 -> binary16 bit pattern, round to nearest even, straight from the 53-bit significand: going through float would round
// twice (a value just above a binary16 tie can land ON the tie in binary32 and then fall to the even side).  Above the largest
// half (65504 + half an ulp) the result is inf, as numpy's astype(float16) gives; NaN stays NaN.
DC_HD uint16_t dc_f64_to_f16_bits(double d) {
  const uint64_t b = dc_bits_of_f64(d);
  const uint16_t sign = (uint16_t)((b >> 48) & 0x8000u);
  const int ex = (int)((b >> 52) & 0x7ff);
  const uint64_t man = b & 0xfffffffffffffull;
  if (ex == 0x7ff) return (uint16_t)(sign | 0x7c00u | (man ? (0x200u | (unsigned)(man >> 42)) : 0u));
  if (ex == 0) return sign;                                   // zero and binary64 subnormals (< 2^-1022)
  const int e = ex - 1023;
  if (e > 15) return (uint16_t)(sign | 0x7c00u);
  if (e >= -14) {                                             // normal half; a carry out of the mantissa walks into the exponent (-> inf at the top)
    unsigned h = ((unsigned)(e + 15) << 10) | (unsigned)(man >> 42);
    const uint64_t rem = man & ((1ull << 42) - 1), half = 1ull << 41;
    if (rem > half || (rem == half && (h & 1u))) ++h;
    return (uint16_t)(sign | h);
  }
  // subnormal half: units of 2^-24.  value = full * 2^(e - 52), so the quotient is full >> (28 - e)
  const int shift = 28 - e;
  if (shift > 54) return sign;                                // below 2^-26: less than half a unit
  const uint64_t full = man | (1ull << 52);
  unsigned h = (unsigned)(full >> shift);
  const uint64_t rem = full & ((1ull << shift) - 1), half = 1ull << (shift - 1);
  if (rem > half || (rem == half && (h & 1u))) ++h;
  return (uint16_t)(sign | h);
}

// binary16 bit pattern -> binary64, exact
DC_HD double dc_f16_bits_to_f64(uint16_t h) {
  const uint64_t sign = (uint64_t)(h & 0x8000u) << 48;
  const unsigned ex = (h >> 10) & 0x1fu, man = h & 0x3ffu;
  if (ex == 0x1f) return dc_f64_of_bits(sign | 0x7ff0000000000000ull | ((uint64_t)man << 42));
  if (ex == 0) {
    if (man == 0) return dc_f64_of_bits(sign);
    const int top = 63 - __builtin_clzll((unsigned long long)man);        // man * 2^-24 = 1.xxx * 2^(top - 24)
    const uint64_t frac = ((uint64_t)man << (52 - top)) & 0xfffffffffffffull;
    return dc_f64_of_bits(sign | ((uint64_t)(top - 24 + 1023) << 52) | frac);
  }
  return dc_f64_of_bits(sign | ((uint64_t)(ex - 15 + 1023) << 52) | ((uint64_t)man << 42));
}

// ---- temporal binning (series.hip, dc_series_bin_time): the mean of b frames rounded half up, floor((2 s + b) / (2 b)) for any b in
// [1, 64] and any sum s of b 16-bit values, negative ones included -- the rule of make_template and dc_motion_bin_round, which
// shifts and so takes powers of two only.  The division is a multiplication by magic = floor(2^32 / 2b) + 1: the numerator is
// first moved by 32768 * 2b to n = 2 s + b + 65536 b, which lies in [b, 3 * 2^22) for |s| <= 65535 b, so the quotient is the
// floor of the signed one plus 32768; and n * magic / 2^32 exceeds n / 2b by less than n / 2^32 < 2^-8 < 1 / 2b, which cannot
// reach the next integer.  tests/native/series_bin_check.cpp holds it against 64-bit floor division.
DC_HD uint32_t dc_series_bin_magic(int b) { return (uint32_t)(0x100000000ull / (uint64_t)(2 * b)) + 1u; }
DC_HD int dc_series_bin_round(int s, int b, uint32_t magic) {
  const uint32_t n = (uint32_t)(2 * s + b + 65536 * b);
  return (int)(uint32_t)(((uint64_t)n * magic) >> 32) - 32768;
}

// ---- signed 128-bit integers from two 64-bit words (two's complement: value = hi * 2^64 + lo) -----------------------------------
struct DcI128 { uint64_t lo; int64_t hi; };

DC_HD DcI128 dc_i128_neg(DcI128 a) {
  DcI128 r;
  r.lo = ~a.lo + 1ull;
  r.hi = (int64_t)(~(uint64_t)a.hi + (r.lo == 0 ? 1ull : 0ull));
  return r;
}
// a * b, exact for every pair of int64
DC_HD DcI128 dc_i128_mul(int64_t a, int64_t b) {
  const bool neg = (a < 0) != (b < 0);
  const uint64_t ua = a < 0 ? 0ull - (uint64_t)a : (uint64_t)a, ub = b < 0 ? 0ull - (uint64_t)b : (uint64_t)b;
  const uint64_t a0 = ua & 0xffffffffull, a1 = ua >> 32, b0 = ub & 0xffffffffull, b1 = ub >> 32;
  const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
  const uint64_t mid = (p00 >> 32) + (p01 & 0xffffffffull) + (p10 & 0xffffffffull);
  DcI128 r;
  r.lo = (p00 & 0xffffffffull) | (mid << 32);
  r.hi = (int64_t)(p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32));
  return neg ? dc_i128_neg(r) : r;
}
// a - b (wraps like any two's complement subtraction; the callers' operands are far inside the range)
DC_HD DcI128 dc_i128_sub(DcI128 a, DcI128 b) {
  DcI128 r;
  r.lo = a.lo - b.lo;
  r.hi = (int64_t)((uint64_t)a.hi - (uint64_t)b.hi - (a.lo < b.lo ? 1ull : 0ull));
  return r;
}
// a + b (wraps like the subtraction)
DC_HD DcI128 dc_i128_add(DcI128 a, DcI128 b) {
  DcI128 r;
  r.lo = a.lo + b.lo;
  r.hi = (int64_t)((uint64_t)a.hi + (uint64_t)b.hi + (r.lo < a.lo ? 1ull : 0ull));
  return r;
}
DC_HD DcI128 dc_i128_from_i64(int64_t a) {
  DcI128 r;
  r.lo = (uint64_t)a;
  r.hi = a < 0 ? -1 : 0;
  return r;
}
// a * b for a 128-bit a and a 64-bit b: the low 128 bits of the product, i.e. exact whenever the product fits (the ROI trace
// kernels, traces.hip: T * sum(S^2) < 2^124).  Magnitudes are multiplied limb by limb, the sign is put back at the end.
DC_HD DcI128 dc_i128_mul_i64(DcI128 a, int64_t b) {
  const bool neg = (a.hi < 0) != (b < 0);
  if (a.hi < 0) a = dc_i128_neg(a);
  const uint64_t ub = b < 0 ? 0ull - (uint64_t)b : (uint64_t)b;
  const uint64_t a0 = a.lo & 0xffffffffull, a1 = a.lo >> 32, b0 = ub & 0xffffffffull, b1 = ub >> 32;
  const uint64_t p00 = a0 * b0, p01 = a0 * b1, p10 = a1 * b0, p11 = a1 * b1;
  const uint64_t mid = (p00 >> 32) + (p01 & 0xffffffffull) + (p10 & 0xffffffffull);
  DcI128 r;
  r.lo = (p00 & 0xffffffffull) | (mid << 32);
  r.hi = (int64_t)(p11 + (p01 >> 32) + (p10 >> 32) + (mid >> 32) + (uint64_t)a.hi * ub);
  return neg ? dc_i128_neg(r) : r;
}
DC_HD bool dc_i128_is_zero(DcI128 a) { return (a.lo | (uint64_t)a.hi) == 0; }
// nearest binary64 (ties to even), ONE rounding: the top 64 bits of the magnitude with a sticky bit for everything below them are
// converted by the uint64 -> double conversion (which rounds to nearest even), then scaled by an exact power of two.
DC_HD double dc_i128_to_f64(DcI128 a) {
  const bool neg = a.hi < 0;
  if (neg) a = dc_i128_neg(a);
  const uint64_t uhi = (uint64_t)a.hi, ulo = a.lo;
  double d;
  if (uhi == 0) {
    d = (double)ulo;
  } else {
    const int lz = __builtin_clzll((unsigned long long)uhi), shift = 64 - lz;
    uint64_t top = lz ? ((uhi << lz) | (ulo >> shift)) : uhi;
    const uint64_t lost = lz ? (ulo << lz) : ulo;
    top |= (lost != 0 ? 1ull : 0ull);
    d = (double)top * dc_f64_of_bits((uint64_t)(1023 + shift) << 52);
  }
  return neg ? -d : d;
}
