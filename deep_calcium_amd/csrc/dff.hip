// dF/F traces on the device (include/dcunet.h, "dF/F traces"): the int64 ROI sums dc_roi_trace_accumulate writes -> the
// neuropil-corrected numerator N (dc_trace_combine), its rolling-percentile baseline B and (N - B) / B (dc_trace_baseline), and
// the per-pixel scalings N / D, B / D (dc_trace_scale).  The reference has no counterpart; the header's definitions are the
// specification.  Integers end to end, one rounding at the end: every float that leaves this file is ONE double division of two
// int64 values, each converted with one round-to-nearest, rounded once more to float32 -- what numpy computes from the same
// integers.  Nothing here may be contracted or reassociated: the pragma below and the per-file flag in _build.py.
#pragma clang fp contract(off)
#include "common.h"
#include "dff_math.h"

namespace {

const int kThreads = 256;
const int kWave = 64;
const int kWaves = kThreads / kWave;
const int kTile = kThreads;                                        // output frames per workgroup pass: one per thread
const int kSpan = kTile + 2 * DC_TRACE_BASELINE_MAX_HALF;          // 4350 staged samples at most: 34800 bytes of LDS
const int kMaxY = 65535;

// num[r][t] = ca[r] * sums[r][t] - cb[r] * sums[np_row[r]][t] + cc[r].  The caller's coefficients keep the result inside int64;
// the arithmetic is done in uint64 so that an out-of-contract input wraps instead of being undefined.
__global__ __launch_bounds__(kThreads) void trace_combine_kernel(const int64_t* __restrict__ sums, long ld, const int* __restrict__ np_row,
                                                                const int64_t* __restrict__ ca, const int64_t* __restrict__ cb,
                                                                const int64_t* __restrict__ cc, long T, int64_t* __restrict__ num) {
  const int r = blockIdx.x;
  const int nr = np_row[r];
  const uint64_t a = (uint64_t)ca[r], b = (uint64_t)cb[r], c = (uint64_t)cc[r];
  const int64_t* own = sums + (long)r * ld;
  const int64_t* ring = nr >= 0 ? sums + (long)nr * ld : nullptr;
  for (long t = (long)blockIdx.y * kThreads + threadIdx.x; t < T; t += (long)gridDim.y * kThreads) {
    uint64_t v = a * (uint64_t)own[t] + c;
    if (ring) v -= b * (uint64_t)ring[t];
    num[(long)r * T + t] = (int64_t)v;
  }
}

// out[r][t] = (float)((double)x[r][t] / (double)den[r]); a row whose denominator is not positive is exactly 0
__global__ __launch_bounds__(kThreads) void trace_scale_kernel(const int64_t* __restrict__ x, long ld, const int64_t* __restrict__ den, long T,
                                                              float* __restrict__ out) {
  const int r = blockIdx.x;
  const int64_t d = den[r];
  const double dd = (double)d;
  const int64_t* row = x + (long)r * ld;
  for (long t = (long)blockIdx.y * kThreads + threadIdx.x; t < T; t += (long)gridDim.y * kThreads)
    out[(long)r * T + t] = d > 0 ? (float)((double)row[t] / dd) : 0.f;
}

__device__ __forceinline__ int64_t wave_min(int64_t v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const int64_t w = (int64_t)__shfl_xor((long long)v, o, kWave);
    v = w < v ? w : v;
  }
  return v;
}
__device__ __forceinline__ int64_t wave_max(int64_t v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const int64_t w = (int64_t)__shfl_xor((long long)v, o, kWave);
    v = w > v ? w : v;
  }
  return v;
}

// One workgroup per (ROI, tile of kTile output frames), striding over the tiles.  The samples every window of the tile can reach,
// frames [tile0 - half, tile0 + kTile + half) clipped to [0, T), are staged once in LDS.  Thread i owns output frame tile0 + i and
// finds the k-th smallest of its window by bisection on the VALUE: [lo, hi] starts at the staged span's minimum and maximum and
// always holds the answer; a round counts the window's samples <= mid and keeps the half in which the count first reaches
// k + 1.  The count only depends on values, so ties cannot matter, and the number of rounds is ceil(log2(max - min + 1)) at
// most -- 62 bits for the widest input, 20 to 30 for real traces.  In every round lane i reads s[w0_i + j]: neighbouring lanes
// read neighbouring 8-byte words, or the same word where the windows are clipped at the start of the trace (a broadcast).
__global__ __launch_bounds__(kThreads) void trace_baseline_kernel(const int64_t* __restrict__ num, long ld, long T, int half, int q, int tiles,
                                                                 int64_t* __restrict__ base, float* __restrict__ dff) {
  __shared__ int64_t s[kSpan];
  __shared__ int64_t red_lo[kWaves], red_hi[kWaves];
  const int r = blockIdx.x, tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
  const int64_t* row = num + (long)r * ld;
  for (int tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
    const long tile0 = (long)tile * kTile;                            // < T: the span below is never empty
    const long a = tile0 - half > 0 ? tile0 - half : 0;
    const long b = tile0 + kTile + half < T ? tile0 + kTile + half : T;
    const int m = (int)(b - a);                                       // <= kSpan
    __syncthreads();                                                  // the readers of the previous tile are done
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    for (int i = tid; i < m; i += kThreads) {
      const int64_t v = row[a + i];
      s[i] = v;
      lo = v < lo ? v : lo;
      hi = v > hi ? v : hi;
    }
    lo = wave_min(lo);
    hi = wave_max(hi);
    if (lane == 0) { red_lo[wave] = lo; red_hi[wave] = hi; }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      lo = red_lo[w] < lo ? red_lo[w] : lo;
      hi = red_hi[w] > hi ? red_hi[w] : hi;
    }
    const long t = tile0 + tid;
    if (t >= T) continue;                                             // no barrier below: the loop's trip count is uniform
    const long w0 = t - half > 0 ? t - half : 0;
    const long w1 = t + half < T - 1 ? t + half : T - 1;
    const int n = (int)(w1 - w0 + 1);
    const int need = dc_dff_rank(q, n) + 1;                           // samples that are <= the k-th smallest: at least k + 1
    const int64_t* w = s + (w0 - a);
    while (lo < hi) {
      const int64_t mid = dc_dff_midpoint(lo, hi);                    // lo <= mid < hi
      int c = 0;
      for (int j = 0; j < n; ++j) c += w[j] <= mid ? 1 : 0;
      if (c >= need) hi = mid;
      else lo = mid + 1;
    }
    const int64_t v = s[t - a];
    if (base) base[(long)r * T + t] = lo;
    if (dff) dff[(long)r * T + t] = lo > 0 ? (float)((double)(v - lo) / (double)lo) : 0.f;
  }
}

}  // namespace

extern "C" int dc_trace_combine(const long* sums, long ld, const int* np_row, const long* ca, const long* cb, const long* cc, int R, long T,
                                long* num, dc_stream_t stream) {
  DC_REQUIRE(sums && np_row && ca && cb && cc && num, DC_EINVAL, "dc_trace_combine: null pointer");
  DC_REQUIRE(R >= 0 && T >= 0, DC_EINVAL, "dc_trace_combine: negative count (R %d, T %ld)", R, T);
  DC_REQUIRE(ld >= T, DC_EINVAL, "dc_trace_combine: ld = %ld is below T = %ld", ld, T);
  DC_REQUIRE((((uintptr_t)sums | (uintptr_t)ca | (uintptr_t)cb | (uintptr_t)cc | (uintptr_t)num) & 7) == 0 && (((uintptr_t)np_row) & 3) == 0,
             DC_EINVAL, "dc_trace_combine: misaligned buffer");
  if (R == 0 || T == 0) return DC_OK;
  const long chunks = (T + kThreads - 1) / kThreads;
  const dim3 grid((unsigned)R, (unsigned)(chunks < kMaxY ? chunks : kMaxY));
  hipLaunchKernelGGL(trace_combine_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, (const int64_t*)sums, ld, np_row, (const int64_t*)ca,
                     (const int64_t*)cb, (const int64_t*)cc, T, (int64_t*)num);
  DC_CHECK_LAUNCH("dc_trace_combine");
  return DC_OK;
}

extern "C" int dc_trace_baseline(const long* num, long ld, int R, long T, int half, int q, long* base, float* dff, dc_stream_t stream) {
  DC_REQUIRE(num, DC_EINVAL, "dc_trace_baseline: null pointer");
  DC_REQUIRE(R >= 0 && T >= 0 && half >= 0, DC_EINVAL, "dc_trace_baseline: negative count (R %d, T %ld, half %d)", R, T, half);
  DC_REQUIRE(q >= 0 && q <= 100, DC_EINVAL, "dc_trace_baseline: percentile q = %d is outside [0, 100]", q);
  DC_REQUIRE(ld >= T, DC_EINVAL, "dc_trace_baseline: ld = %ld is below T = %ld", ld, T);
  DC_REQUIRE((((uintptr_t)num | (uintptr_t)base) & 7) == 0 && (((uintptr_t)dff) & 3) == 0, DC_EINVAL, "dc_trace_baseline: misaligned buffer");
  DC_REQUIRE(half <= DC_TRACE_BASELINE_MAX_HALF, DC_EUNSUP, "dc_trace_baseline: half = %d: the window half-width is limited to %d", half,
             DC_TRACE_BASELINE_MAX_HALF);
  if (R == 0 || T == 0 || (!base && !dff)) return DC_OK;
  const long tiles = (T + kTile - 1) / kTile;
  DC_REQUIRE(tiles <= INT32_MAX, DC_EUNSUP, "dc_trace_baseline: T = %ld is more frames than the tile index holds", T);
  const dim3 grid((unsigned)R, (unsigned)(tiles < kMaxY ? tiles : kMaxY));
  hipLaunchKernelGGL(trace_baseline_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, (const int64_t*)num, ld, T, half, q, (int)tiles,
                     (int64_t*)base, dff);
  DC_CHECK_LAUNCH("dc_trace_baseline");
  return DC_OK;
}

extern "C" int dc_trace_scale(const long* x, long ld, const long* den, int R, long T, float* out, dc_stream_t stream) {
  DC_REQUIRE(x && den && out, DC_EINVAL, "dc_trace_scale: null pointer");
  DC_REQUIRE(R >= 0 && T >= 0, DC_EINVAL, "dc_trace_scale: negative count (R %d, T %ld)", R, T);
  DC_REQUIRE(ld >= T, DC_EINVAL, "dc_trace_scale: ld = %ld is below T = %ld", ld, T);
  DC_REQUIRE((((uintptr_t)x | (uintptr_t)den) & 7) == 0 && (((uintptr_t)out) & 3) == 0, DC_EINVAL, "dc_trace_scale: misaligned buffer");
  if (R == 0 || T == 0) return DC_OK;
  const long chunks = (T + kThreads - 1) / kThreads;
  const dim3 grid((unsigned)R, (unsigned)(chunks < kMaxY ? chunks : kMaxY));
  hipLaunchKernelGGL(trace_scale_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, (const int64_t*)x, ld, (const int64_t*)den, T, out);
  DC_CHECK_LAUNCH("dc_trace_scale");
  return DC_OK;
}
