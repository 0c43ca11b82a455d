// ROI trace-pair correlation on the device: for a list of pairs (i, j) of rows of the int64 ROI sums, the exact integer
// numerators N(x_i, x_i), N(x_i, x_j), N(x_j, x_j) of the (segment-pooled) correlation over time, and the float32 correlation --
// what decides whether two neighbouring ROIs are fragments of one cell (include/dcunet.h, "ROI trace-pair correlation").
//
// The sums already lie on the device after the streaming pass (dc_roi_trace_accumulate), so nothing here reads the recording.
// A product of two sums needs up to 112 bits and a numerator up to 124 (trace_pair_math.h derives it): every product is a full
// dc_i128_mul and every accumulator a DcI128.  Nothing in this file may be contracted into a fused multiply-add or reassociated:
// the pragma below and the per-file flag in _build.py.
#pragma clang fp contract(off)
#include "common.h"
#include "trace_pair_math.h"

namespace {

const int kThreads = 256;
const int kWave = 64;
const int kWaves = kThreads / kWave;
const int kLaneSegment = 32;                         // segments shorter than this are walked by one lane each

__device__ __forceinline__ int64_t shfl_xor_i64(int64_t v, int o) { return (int64_t)__shfl_xor((long long)v, o); }

__device__ __forceinline__ DcI128 shfl_xor_i128(DcI128 v, int o) {
  DcI128 r;
  r.lo = (uint64_t)__shfl_xor((unsigned long long)v.lo, o);
  r.hi = (int64_t)__shfl_xor((long long)v.hi, o);
  return r;
}

// the sum over the 64 lanes of a wave, in every lane (integer addition: the order does not matter)
__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += shfl_xor_i64(v, o);
  return v;
}
__device__ __forceinline__ DcI128 wave_sum(DcI128 v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v = dc_i128_add(v, shfl_xor_i128(v, o));
  return v;
}

// the raw sums of two rows over a run of frames
struct Raw {
  int64_t ax, ay;
  DcI128 gxx, gxy, gyy;
};
__device__ __forceinline__ Raw raw_zero() {
  Raw r;
  r.ax = r.ay = 0;
  r.gxx = r.gxy = r.gyy = DcI128{0, 0};
  return r;
}
__device__ __forceinline__ void raw_add(Raw& r, int64_t x, int64_t y) {
  r.ax += x;
  r.ay += y;
  r.gxx = dc_i128_add(r.gxx, dc_i128_mul(x, x));
  r.gxy = dc_i128_add(r.gxy, dc_i128_mul(x, y));
  r.gyy = dc_i128_add(r.gyy, dc_i128_mul(y, y));
}

struct Num { DcI128 xx, xy, yy; };
__device__ __forceinline__ void num_add_segment(Num& n, const Raw& r, int64_t len, int64_t mult) {
  n.xx = dc_i128_add(n.xx, dc_trace_pair_term(len, mult, r.gxx, r.ax, r.ax));
  n.xy = dc_i128_add(n.xy, dc_trace_pair_term(len, mult, r.gxy, r.ax, r.ay));
  n.yy = dc_i128_add(n.yy, dc_trace_pair_term(len, mult, r.gyy, r.ay, r.ay));
}

// One workgroup per pair.  The segments are integers end to end, so who sums what changes no bit; three shapes keep the lanes busy:
//   one segment (n == 1): the 256 lanes stride along t, both rows read coalesced; the raw sums are reduced over the wave by
//     shuffles and over the four waves through LDS, and thread 0 forms the term;
//   segments of at least kLaneSegment frames: one wave per segment, its lanes striding along t, reduced by shuffles, lane 0 forms
//     the term and keeps its wave's share of N;
//   shorter segments: one lane per segment (neighbouring lanes read neighbouring runs of the rows), the lane forms the term.
// Every thread then holds a share of {Nxx, Nxy, Nyy} (zero for most); the shares are added over the wave and the waves, and
// thread 0 alone writes the pair's six words.  No atomics; the float step is dc_trace_pair_corr's, in one place.
__global__ __launch_bounds__(kThreads) void trace_pair_moments_kernel(const int64_t* __restrict__ sums, long ld, int R, int64_t T, int seg_len,
                                                                     const int* __restrict__ pairs, int64_t* __restrict__ num) {
  __shared__ int64_t red[kWaves][8];
  const long p = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int i = pairs[2 * p], j = pairs[2 * p + 1];
  int64_t* out = num + 6 * p;
  if (i < 0 || i >= R || j < 0 || j >= R) {          // uniform over the workgroup: a pair that names no row gets zeros
    if (tid == 0)
      for (int k = 0; k < 6; ++k) out[k] = 0;
    return;
  }
  const int64_t* __restrict__ x = sums + (long)i * ld;
  const int64_t* __restrict__ y = sums + (long)j * ld;
  const DcTracePairPlan plan = dc_trace_pair_plan(T, seg_len);
  Num mine = {{0, 0}, {0, 0}, {0, 0}};
  if (plan.n == 1) {
    Raw r = raw_zero();
    for (int64_t t = tid; t < T; t += kThreads) raw_add(r, x[t], y[t]);
    r.ax = wave_sum(r.ax); r.ay = wave_sum(r.ay);
    r.gxx = wave_sum(r.gxx); r.gxy = wave_sum(r.gxy); r.gyy = wave_sum(r.gyy);
    if (lane == 0) {
      int64_t* w = red[wave];
      w[0] = r.ax; w[1] = r.ay;
      w[2] = (int64_t)r.gxx.lo; w[3] = r.gxx.hi; w[4] = (int64_t)r.gxy.lo; w[5] = r.gxy.hi; w[6] = (int64_t)r.gyy.lo; w[7] = r.gyy.hi;
    }
    __syncthreads();
    if (tid == 0) {
      Raw s = raw_zero();
      for (int k = 0; k < kWaves; ++k) {
        const int64_t* w = red[k];
        s.ax += w[0]; s.ay += w[1];
        s.gxx = dc_i128_add(s.gxx, DcI128{(uint64_t)w[2], w[3]});
        s.gxy = dc_i128_add(s.gxy, DcI128{(uint64_t)w[4], w[5]});
        s.gyy = dc_i128_add(s.gyy, DcI128{(uint64_t)w[6], w[7]});
      }
      num_add_segment(mine, s, T, 1);
    }
    __syncthreads();                                 // red is reused below
  } else if (plan.L >= kLaneSegment) {
    for (int64_t s = wave; s < plan.n; s += kWaves) {
      int64_t start, len, mult;
      dc_trace_pair_segment(plan, s, &start, &len, &mult);
      Raw r = raw_zero();
      for (int64_t t = lane; t < len; t += kWave) raw_add(r, x[start + t], y[start + t]);
      r.ax = wave_sum(r.ax); r.ay = wave_sum(r.ay);
      r.gxx = wave_sum(r.gxx); r.gxy = wave_sum(r.gxy); r.gyy = wave_sum(r.gyy);
      if (lane == 0) num_add_segment(mine, r, len, mult);
    }
  } else {
    for (int64_t s = tid; s < plan.n; s += kThreads) {
      int64_t start, len, mult;
      dc_trace_pair_segment(plan, s, &start, &len, &mult);
      Raw r = raw_zero();
      for (int64_t t = 0; t < len; ++t) raw_add(r, x[start + t], y[start + t]);
      num_add_segment(mine, r, len, mult);
    }
  }
  mine.xx = wave_sum(mine.xx); mine.xy = wave_sum(mine.xy); mine.yy = wave_sum(mine.yy);
  if (lane == 0) {
    int64_t* w = red[wave];
    w[0] = (int64_t)mine.xx.lo; w[1] = mine.xx.hi; w[2] = (int64_t)mine.xy.lo; w[3] = mine.xy.hi; w[4] = (int64_t)mine.yy.lo; w[5] = mine.yy.hi;
  }
  __syncthreads();
  if (tid == 0) {
    Num n = {{0, 0}, {0, 0}, {0, 0}};
    for (int k = 0; k < kWaves; ++k) {
      const int64_t* w = red[k];
      n.xx = dc_i128_add(n.xx, DcI128{(uint64_t)w[0], w[1]});
      n.xy = dc_i128_add(n.xy, DcI128{(uint64_t)w[2], w[3]});
      n.yy = dc_i128_add(n.yy, DcI128{(uint64_t)w[4], w[5]});
    }
    out[0] = (int64_t)n.xx.lo; out[1] = n.xx.hi; out[2] = (int64_t)n.xy.lo; out[3] = n.xy.hi; out[4] = (int64_t)n.yy.lo; out[5] = n.yy.hi;
  }
}

// numerators -> float32, one thread per pair
__global__ __launch_bounds__(kThreads) void trace_pair_corr_kernel(const int64_t* __restrict__ num, long P, float* __restrict__ corr) {
  const long p = (long)blockIdx.x * kThreads + threadIdx.x;
  if (p >= P) return;
  const int64_t* w = num + 6 * p;
  DcFpNum n;
  n.cxx = DcI128{(uint64_t)w[0], w[1]};
  n.cxl = DcI128{(uint64_t)w[2], w[3]};
  n.cll = DcI128{(uint64_t)w[4], w[5]};
  corr[p] = dc_fp_corr(n);
}

}  // namespace

extern "C" int dc_trace_pair_moments(const long* sums, long ld, int R, long T, int seg_len, const int* pairs, long P, long* num,
                                     dc_stream_t stream) {
  DC_REQUIRE(sums && pairs && num, DC_EINVAL, "dc_trace_pair_moments: null pointer");
  DC_REQUIRE(R >= 0 && T >= 0 && P >= 0, DC_EINVAL, "dc_trace_pair_moments: negative count (R %d, T %ld, P %ld)", R, T, P);
  DC_REQUIRE(ld >= T, DC_EINVAL, "dc_trace_pair_moments: ld = %ld is below T = %ld", ld, T);
  DC_REQUIRE((((uintptr_t)sums | (uintptr_t)num) & 7) == 0 && (((uintptr_t)pairs) & 3) == 0, DC_EINVAL,
             "dc_trace_pair_moments: misaligned buffer");
  DC_REQUIRE(seg_len == 0 || seg_len >= DC_DETREND_MIN_FRAMES, DC_EINVAL,
             "dc_trace_pair_moments: seg_len = %d: 0 (one segment) or a segment of at least %d frames", seg_len, DC_DETREND_MIN_FRAMES);
  DC_REQUIRE(seg_len <= DC_DETREND_MAX_FRAMES, DC_EUNSUP, "dc_trace_pair_moments: seg_len = %d: a segment is limited to %d frames", seg_len,
             DC_DETREND_MAX_FRAMES);
  DC_REQUIRE(T <= DC_ROI_PIXEL_MAX_FRAMES, DC_EUNSUP, "dc_trace_pair_moments: T = %ld: T is limited to 2^31 - 1 = %ld", T,
             (long)DC_ROI_PIXEL_MAX_FRAMES);
  DC_REQUIRE(P <= DC_TRACE_PAIR_MAX_PAIRS, DC_EUNSUP, "dc_trace_pair_moments: P = %ld pairs: limited to 2^24 = %ld", P,
             (long)DC_TRACE_PAIR_MAX_PAIRS);
  if (P == 0 || R == 0 || T == 0) return DC_OK;
  hipLaunchKernelGGL(trace_pair_moments_kernel, dim3((unsigned)P), dim3(kThreads), 0, (hipStream_t)stream, (const int64_t*)sums, ld, R,
                     (int64_t)T, seg_len, pairs, (int64_t*)num);
  DC_CHECK_LAUNCH("dc_trace_pair_moments");
  return DC_OK;
}

extern "C" int dc_trace_pair_corr(const long* num, long P, float* corr, dc_stream_t stream) {
  DC_REQUIRE(num && corr, DC_EINVAL, "dc_trace_pair_corr: null pointer");
  DC_REQUIRE(P >= 0, DC_EINVAL, "dc_trace_pair_corr: negative count (P %ld)", P);
  DC_REQUIRE((((uintptr_t)num) & 7) == 0 && (((uintptr_t)corr) & 3) == 0, DC_EINVAL, "dc_trace_pair_corr: misaligned buffer");
  DC_REQUIRE(P <= DC_TRACE_PAIR_MAX_PAIRS, DC_EUNSUP, "dc_trace_pair_corr: P = %ld pairs: limited to 2^24 = %ld", P,
             (long)DC_TRACE_PAIR_MAX_PAIRS);
  if (P == 0) return DC_OK;
  hipLaunchKernelGGL(trace_pair_corr_kernel, dim3((unsigned)dc_cdiv(P, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                     (const int64_t*)num, P, corr);
  DC_CHECK_LAUNCH("dc_trace_pair_corr");
  return DC_OK;
}
