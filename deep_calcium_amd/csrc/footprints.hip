// ROI footprint maps on the device: for every ROI and every pixel of its support (the ROI's pixels plus a halo), the correlation
// over time of the pixel's series x(t) with the ROI's own trace S(t) -- what tells a neuron from a static bright structure, and a
// pixel of the cell from a pixel of the neuropil beside it (include/dcunet.h, "ROI footprint maps").
//
// One pass over the recording beside dc_roi_trace_accumulate gathers the exact integer moments a = sum x, b = sum x^2,
// c = sum x S of every support entry; dc_roi_trace_moments reduces u = sum S, w = sum S^2 per ROI; dc_roi_pixel_corr forms the
// numerators in 128-bit integers (footprint_math.h) and rounds once.  Nothing in this file may be contracted into a fused
// multiply-add or reassociated: the pragma below and the per-file flag in _build.py.
#pragma clang fp contract(off)
#include "common.h"
#include "footprint_math.h"
#include "detrend_math.h"

namespace {

const int kThreads = 256;
const int kFpw = 8;                   // frames whose 2-byte gathers a lane keeps in flight
// Frames of the ROI's trace staged in LDS at a time, and the run of frames over which a lane sums x * S_lo and x * S_hi in int64
// before folding them into its 128-bit c: |x| < 2^16 and S_lo < 2^32 give |x * S_lo| < 2^48, so a run of 512 stays below 2^57
// (anything up to 2^15 - 1 frames would fit int64); S_hi is an int32 for EVERY int64 S, |x * S_hi| < 2^47, a run below 2^56.
const int kStage = 512;

template <bool UNS>
__device__ __forceinline__ int widen(uint16_t v) { return UNS ? (int)v : (int)(int16_t)v; }

// One workgroup per CSR row of the support, one LANE per entry: lane i of a batch of kThreads consecutive entries owns entry
// p0 + i for the whole chunk, so its four words of state are read once, kept in registers and written once, by this thread alone
// -- no atomics, no partial sums whose grouping depends on the grid.  Consecutive entries of a support are consecutive flat
// indices along an image row (the support is sorted), so the 64 gathers of a wave-instruction fall into a few 128-byte lines of
// one frame, as in roi_trace_accumulate_kernel; kFpw frames are in flight per lane.  The row's ROI trace for the staged frames
// sits in LDS (every lane reads the same word: a broadcast, no bank conflict).
template <bool UNS>
__global__ __launch_bounds__(kThreads) void roi_pixel_accumulate_kernel(const uint16_t* __restrict__ frames, int tc, long t0,
                                                                       const int* __restrict__ row_off, const int* __restrict__ row_pix,
                                                                       const int* __restrict__ row_roi, int R,
                                                                       const int64_t* __restrict__ sums, long ld, int64_t* __restrict__ mom,
                                                                       long N, long HW) {
  __shared__ int64_t ss[kStage];
  const int s = blockIdx.x, tid = threadIdx.x;
  const int r = row_roi ? row_roi[s] : s;
  if (r < 0 || r >= R) return;                       // the whole workgroup: a row that names no ROI has no trace to compare with
  long a0 = row_off[s], b0 = row_off[s + 1];
  if (a0 < 0) a0 = 0;
  if (b0 > N) b0 = N;                                // an entry beyond the state is never touched
  const int64_t* srow = sums + (long)r * ld + t0;
  for (long p0 = a0; p0 < b0; p0 += kThreads) {
    const long e = p0 + tid;
    int q = e < b0 ? row_pix[e] : -1;
    if (q < 0 || q >= HW) q = -1;                    // sanitised: never dereferenced, contributes nothing
    int64_t sa = 0, sb = 0;
    DcI128 c = {0, 0};
    for (int f0 = 0; f0 < tc; f0 += kStage) {
      const int nst = tc - f0 < kStage ? tc - f0 : kStage;
      __syncthreads();                               // the readers of the previous stage are done
      for (int i = tid; i < kStage; i += kThreads) ss[i] = i < nst ? srow[f0 + i] : 0;
      __syncthreads();
      const uint16_t* f = frames + (long)f0 * HW + (q < 0 ? 0 : q);
      int64_t lo = 0, hi = 0;
      for (int k0 = 0; q >= 0 && k0 < nst; k0 += kFpw) {       // (the barriers are outside: every thread reaches them)
        int v[kFpw];
#pragma unroll
        for (int k = 0; k < kFpw; ++k) v[k] = k0 + k < nst ? widen<UNS>(f[(long)(k0 + k) * HW]) : 0;
#pragma unroll
        for (int k = 0; k < kFpw; ++k) {
          const int64_t x = v[k];
          uint32_t slo;
          int32_t shi;
          dc_fp_split(ss[k0 + k], &slo, &shi);       // k0 + k < kStage (a multiple of kFpw); beyond nst x is 0
          sa += x;
          sb += x * x;
          lo += x * (int64_t)slo;
          hi += x * (int64_t)shi;
        }
      }
      c = dc_fp_fold(c, lo, hi);
    }
    if (q < 0) continue;
    mom[e] += sa;
    mom[N + e] += sb;
    DcI128 st;
    st.lo = (uint64_t)mom[2 * N + e];
    st.hi = mom[3 * N + e];
    st = dc_i128_add(st, c);
    mom[2 * N + e] = (int64_t)st.lo;
    mom[3 * N + e] = st.hi;
  }
}

// u = sum S, w = sum S^2 of every ROI's trace, one workgroup per ROI: the reduction of roi_trace_finalize_kernel (a fixed tree, and
// integer addition: the order does not matter).
__global__ __launch_bounds__(kThreads) void roi_trace_moments_kernel(const int64_t* __restrict__ sums, long ld, int64_t T, int R,
                                                                    int64_t* __restrict__ rmom) {
  __shared__ int64_t sm1[kThreads];
  __shared__ uint64_t sm2lo[kThreads];
  __shared__ int64_t sm2hi[kThreads];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int64_t* row = sums + (long)r * ld;
  int64_t s1 = 0;
  DcI128 s2 = {0, 0};
  for (int64_t t = tid; t < T; t += kThreads) {
    const int64_t v = row[t];
    s1 += v;
    s2 = dc_i128_add(s2, dc_i128_mul(v, v));
  }
  sm1[tid] = s1; sm2lo[tid] = s2.lo; sm2hi[tid] = s2.hi;
  __syncthreads();
  for (int k = kThreads / 2; k > 0; k >>= 1) {
    if (tid < k) {
      DcI128 x = {sm2lo[tid], sm2hi[tid]}, y = {sm2lo[tid + k], sm2hi[tid + k]};
      x = dc_i128_add(x, y);
      sm1[tid] += sm1[tid + k]; sm2lo[tid] = x.lo; sm2hi[tid] = x.hi;
    }
    __syncthreads();
  }
  if (tid == 0) {
    rmom[r] = sm1[0];
    rmom[(long)R + r] = (int64_t)sm2lo[0];
    rmom[2L * R + r] = sm2hi[0];
  }
}

// moments -> the float32 map, one workgroup per CSR row, one lane per entry
__global__ __launch_bounds__(kThreads) void roi_pixel_corr_kernel(const int64_t* __restrict__ mom, long N, const int* __restrict__ row_off,
                                                                 const int* __restrict__ row_roi, int R, const int* __restrict__ inside,
                                                                 const int64_t* __restrict__ rmom, int64_t T, float* __restrict__ corr) {
  const int s = blockIdx.x;
  const int r = row_roi ? row_roi[s] : s;
  long a0 = row_off[s], b0 = row_off[s + 1];
  if (a0 < 0) a0 = 0;
  if (b0 > N) b0 = N;
  const bool named = r >= 0 && r < R;
  int64_t u = 0;
  DcI128 w = {0, 0};
  if (named) {
    u = rmom[r];
    w.lo = (uint64_t)rmom[(long)R + r];
    w.hi = rmom[2L * R + r];
  }
  for (long e = a0 + threadIdx.x; e < b0; e += kThreads) {
    float out = 0.f;                                 // a row that names no ROI: 0
    if (named) {
      DcI128 c;
      c.lo = (uint64_t)mom[2 * N + e];
      c.hi = mom[3 * N + e];
      out = dc_fp_corr(dc_fp_numerators(T, mom[e], mom[N + e], c, u, w, inside[e] != 0));
    }
    corr[e] = out;
  }
}

// ---- detrended footprints: segment-pooled centred moments (include/dcunet.h, "Detrended correlations") -----------------------------
// One workgroup per CSR row, one lane per entry, as in the accumulate kernel: the lane alone owns the entry's two pooled words and
// its four planes of mom, which it folds with its ROI's segment moments (u, w of dc_roi_trace_moments over the segment's columns)
// and clears for the next segment.
__global__ __launch_bounds__(kThreads) void roi_pixel_fold_segment_kernel(int64_t* __restrict__ mom, long N, const int* __restrict__ row_off,
                                                                         const int* __restrict__ row_roi, int R,
                                                                         const int64_t* __restrict__ rmom, int64_t len, int64_t mult,
                                                                         int64_t* __restrict__ pxx, int64_t* __restrict__ pxs) {
  const int s = blockIdx.x;
  const int r = row_roi ? row_roi[s] : s;
  if (r < 0 || r >= R) return;                       // the accumulate kernel added nothing to such a row
  long a0 = row_off[s], b0 = row_off[s + 1];
  if (a0 < 0) a0 = 0;
  if (b0 > N) b0 = N;
  const int64_t u = rmom[r];
  for (long e = a0 + threadIdx.x; e < b0; e += kThreads) {
    const int64_t a = mom[e];
    DcI128 c;
    c.lo = (uint64_t)mom[2 * N + e];
    c.hi = mom[3 * N + e];
    dc_i128_store(pxx, e, dc_i128_add(dc_i128_load(pxx, e), dc_detrend_term(len, mult, mom[N + e], a, a)));
    dc_i128_store(pxs, e, dc_i128_add(dc_i128_load(pxs, e), dc_detrend_term_wide(len, mult, c, a, u)));
    mom[e] = 0; mom[N + e] = 0; mom[2 * N + e] = 0; mom[3 * N + e] = 0;
  }
}

// the ROI's own pooled Css, one lane per ROI
__global__ __launch_bounds__(kThreads) void roi_trace_fold_segment_kernel(const int64_t* __restrict__ rmom, int R, int64_t len, int64_t mult,
                                                                         int64_t* __restrict__ pss) {
  const long r = (long)blockIdx.x * kThreads + threadIdx.x;
  if (r >= R) return;
  const int64_t u = rmom[r];
  DcI128 w;
  w.lo = (uint64_t)rmom[(long)R + r];
  w.hi = rmom[2L * R + r];
  dc_i128_store(pss, r, dc_i128_add(dc_i128_load(pss, r), dc_detrend_term_wide(len, mult, w, u, u)));
}

// pooled numerators -> the float32 map, in the form of roi_pixel_corr_kernel
__global__ __launch_bounds__(kThreads) void roi_pixel_corr_pooled_kernel(const int64_t* __restrict__ pxx, const int64_t* __restrict__ pxs,
                                                                        const int64_t* __restrict__ pss, long N,
                                                                        const int* __restrict__ row_off, const int* __restrict__ row_roi,
                                                                        int R, const int* __restrict__ inside, float* __restrict__ corr) {
  const int s = blockIdx.x;
  const int r = row_roi ? row_roi[s] : s;
  long a0 = row_off[s], b0 = row_off[s + 1];
  if (a0 < 0) a0 = 0;
  if (b0 > N) b0 = N;
  const bool named = r >= 0 && r < R;
  DcI128 css = {0, 0};
  if (named) css = dc_i128_load(pss, r);
  for (long e = a0 + threadIdx.x; e < b0; e += kThreads)
    corr[e] = named ? dc_fp_corr(dc_detrend_fp_numerators(dc_i128_load(pxx, e), dc_i128_load(pxs, e), css, inside[e] != 0)) : 0.f;
}

}  // namespace

extern "C" int dc_roi_pixel_fold_segment(long* mom, int N, const int* row_off, const int* row_roi, int S, int R, const long* rmom, long len,
                                         long mult, long* pooled_xx, long* pooled_xs, long* pooled_ss, int H, int W, dc_stream_t stream) {
  DC_REQUIRE(mom && row_off && rmom && pooled_xx && pooled_xs && pooled_ss, DC_EINVAL, "dc_roi_pixel_fold_segment: null pointer");
  DC_REQUIRE(N >= 0 && S >= 0 && R >= 0, DC_EINVAL, "dc_roi_pixel_fold_segment: negative count (N %d, S %d, R %d)", N, S, R);
  DC_REQUIRE(row_roi || S == R, DC_EINVAL, "dc_roi_pixel_fold_segment: without row_roi every CSR row is an ROI, but S = %d and R = %d", S, R);
  DC_REQUIRE((((uintptr_t)mom | (uintptr_t)rmom) & 7) == 0 && (((uintptr_t)row_off | (uintptr_t)row_roi) & 3) == 0 && dc_aligned16(pooled_xx) &&
             dc_aligned16(pooled_xs) && dc_aligned16(pooled_ss), DC_EINVAL,
             "dc_roi_pixel_fold_segment: misaligned buffer (the pooled words are 16-byte elements)");
  DC_REQUIRE(H > 0 && W > 0 && (long)H * W <= (1L << 30), DC_EINVAL, "dc_roi_pixel_fold_segment: image %d x %d out of range", H, W);
  DC_REQUIRE(len >= 1 && mult >= 1, DC_EINVAL, "dc_roi_pixel_fold_segment: a segment of %ld frames with mult %ld", len, mult);
  DC_REQUIRE(dc_detrend_segment_ok(len, mult), DC_EUNSUP,
             "dc_roi_pixel_fold_segment: len = %ld, mult = %ld: a segment beside others is limited to %d frames, one alone to %ld", len, mult,
             DC_DETREND_MAX_SEGMENT, (long)DC_ROI_PIXEL_MAX_FRAMES);
  DC_REQUIRE(dc_detrend_volume_ok(len, mult, (long)H * W), DC_EUNSUP,
             "dc_roi_pixel_fold_segment: M = %ld on %d x %d: M * H * W is limited to 2^46", len * mult, H, W);
  if (R == 0) return DC_OK;
  hipLaunchKernelGGL(roi_trace_fold_segment_kernel, dim3((unsigned)dc_cdiv((long)R, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                     (const int64_t*)rmom, R, (int64_t)len, (int64_t)mult, (int64_t*)pooled_ss);
  DC_CHECK_LAUNCH("dc_roi_pixel_fold_segment(rois)");
  if (N == 0 || S == 0) return DC_OK;
  hipLaunchKernelGGL(roi_pixel_fold_segment_kernel, dim3((unsigned)S), dim3(kThreads), 0, (hipStream_t)stream, (int64_t*)mom, (long)N, row_off,
                     row_roi, R, (const int64_t*)rmom, (int64_t)len, (int64_t)mult, (int64_t*)pooled_xx, (int64_t*)pooled_xs);
  DC_CHECK_LAUNCH("dc_roi_pixel_fold_segment");
  return DC_OK;
}

extern "C" int dc_roi_pixel_corr_pooled(const long* pooled_xx, const long* pooled_xs, const long* pooled_ss, int N, const int* row_off,
                                        const int* row_roi, int S, int R, const int* inside, float* corr, dc_stream_t stream) {
  DC_REQUIRE(pooled_xx && pooled_xs && pooled_ss && row_off && inside && corr, DC_EINVAL, "dc_roi_pixel_corr_pooled: null pointer");
  DC_REQUIRE(N >= 0 && S >= 0 && R >= 0, DC_EINVAL, "dc_roi_pixel_corr_pooled: negative count (N %d, S %d, R %d)", N, S, R);
  DC_REQUIRE(row_roi || S == R, DC_EINVAL, "dc_roi_pixel_corr_pooled: without row_roi every CSR row is an ROI, but S = %d and R = %d", S, R);
  DC_REQUIRE(dc_aligned16(pooled_xx) && dc_aligned16(pooled_xs) && dc_aligned16(pooled_ss) &&
             (((uintptr_t)row_off | (uintptr_t)row_roi | (uintptr_t)inside | (uintptr_t)corr) & 3) == 0, DC_EINVAL,
             "dc_roi_pixel_corr_pooled: misaligned buffer (the pooled words are 16-byte elements)");
  if (N == 0 || S == 0) return DC_OK;
  hipLaunchKernelGGL(roi_pixel_corr_pooled_kernel, dim3((unsigned)S), dim3(kThreads), 0, (hipStream_t)stream, (const int64_t*)pooled_xx,
                     (const int64_t*)pooled_xs, (const int64_t*)pooled_ss, (long)N, row_off, row_roi, R, inside, corr);
  DC_CHECK_LAUNCH("dc_roi_pixel_corr_pooled");
  return DC_OK;
}

extern "C" int dc_roi_pixel_accumulate(const void* frames, int is_unsigned, int tc, long t0, const int* row_off, const int* row_pix,
                                       const int* row_roi, int S, int R, const long* sums, long ld, long* mom, int N, int H, int W,
                                       dc_stream_t stream) {
  DC_REQUIRE(frames && row_off && row_pix && sums && mom, DC_EINVAL, "dc_roi_pixel_accumulate: null pointer");
  DC_REQUIRE(S >= 0 && R >= 0 && N >= 0 && tc >= 0 && t0 >= 0, DC_EINVAL,
             "dc_roi_pixel_accumulate: negative count (S %d, R %d, N %d, tc %d, t0 %ld)", S, R, N, tc, t0);
  DC_REQUIRE_FRAMES("dc_roi_pixel_accumulate", tc);
  DC_REQUIRE(row_roi || S == R, DC_EINVAL, "dc_roi_pixel_accumulate: without row_roi every CSR row is an ROI, but S = %d and R = %d", S, R);
  DC_REQUIRE(ld >= t0 + tc, DC_EINVAL, "dc_roi_pixel_accumulate: ld = %ld is below t0 + tc = %ld", ld, t0 + tc);
  DC_REQUIRE(H > 0 && W > 0 && (long)H * W <= (1L << 30), DC_EINVAL, "dc_roi_pixel_accumulate: image %d x %d out of range", H, W);
  DC_REQUIRE((((uintptr_t)frames) & 1) == 0 && (((uintptr_t)row_off | (uintptr_t)row_pix | (uintptr_t)row_roi) & 3) == 0 &&
             (((uintptr_t)sums | (uintptr_t)mom) & 7) == 0, DC_EINVAL, "dc_roi_pixel_accumulate: misaligned buffer");
  const long HW = (long)H * W;
  DC_REQUIRE(t0 + tc <= DC_ROI_TRACE_MAX_VOLUME / HW, DC_EUNSUP,
             "dc_roi_pixel_accumulate: %ld frames of %d x %d: T * H * W is limited to 2^46 = %ld", t0 + tc, H, W, (long)DC_ROI_TRACE_MAX_VOLUME);
  DC_REQUIRE(t0 + tc <= DC_ROI_PIXEL_MAX_FRAMES, DC_EUNSUP, "dc_roi_pixel_accumulate: %ld frames: T is limited to 2^31 - 1 = %ld", t0 + tc,
             (long)DC_ROI_PIXEL_MAX_FRAMES);
  if (N == 0 || S == 0 || R == 0 || tc == 0) return DC_OK;
  const dim3 grid((unsigned)S), block(kThreads);
  const uint16_t* f = (const uint16_t*)frames;
  if (is_unsigned)
    hipLaunchKernelGGL((roi_pixel_accumulate_kernel<true>), grid, block, 0, (hipStream_t)stream, f, tc, t0, row_off, row_pix, row_roi, R,
                       (const int64_t*)sums, ld, (int64_t*)mom, (long)N, HW);
  else
    hipLaunchKernelGGL((roi_pixel_accumulate_kernel<false>), grid, block, 0, (hipStream_t)stream, f, tc, t0, row_off, row_pix, row_roi, R,
                       (const int64_t*)sums, ld, (int64_t*)mom, (long)N, HW);
  DC_CHECK_LAUNCH("dc_roi_pixel_accumulate");
  return DC_OK;
}

extern "C" int dc_roi_trace_moments(const long* sums, long ld, int R, long T, long* rmom, dc_stream_t stream) {
  DC_REQUIRE(sums && rmom, DC_EINVAL, "dc_roi_trace_moments: null pointer");
  DC_REQUIRE(R >= 0 && T >= 0, DC_EINVAL, "dc_roi_trace_moments: negative count (R %d, T %ld)", R, T);
  DC_REQUIRE(ld >= T, DC_EINVAL, "dc_roi_trace_moments: ld = %ld is below T = %ld", ld, T);
  DC_REQUIRE((((uintptr_t)sums | (uintptr_t)rmom) & 7) == 0, DC_EINVAL, "dc_roi_trace_moments: misaligned buffer");
  DC_REQUIRE(T <= DC_ROI_PIXEL_MAX_FRAMES, DC_EUNSUP, "dc_roi_trace_moments: T = %ld: T is limited to 2^31 - 1 = %ld", T,
             (long)DC_ROI_PIXEL_MAX_FRAMES);
  if (R == 0) return DC_OK;                          // T == 0 still writes u = w = 0
  hipLaunchKernelGGL(roi_trace_moments_kernel, dim3((unsigned)R), dim3(kThreads), 0, (hipStream_t)stream, (const int64_t*)sums, ld,
                     (int64_t)T, R, (int64_t*)rmom);
  DC_CHECK_LAUNCH("dc_roi_trace_moments");
  return DC_OK;
}

extern "C" int dc_roi_pixel_corr(const long* mom, int N, const int* row_off, const int* row_roi, int S, int R, const int* inside,
                                 const long* rmom, long T, float* corr, dc_stream_t stream) {
  DC_REQUIRE(mom && row_off && inside && rmom && corr, DC_EINVAL, "dc_roi_pixel_corr: null pointer");
  DC_REQUIRE(N >= 0 && S >= 0 && R >= 0 && T >= 0, DC_EINVAL, "dc_roi_pixel_corr: negative count (N %d, S %d, R %d, T %ld)", N, S, R, T);
  DC_REQUIRE(row_roi || S == R, DC_EINVAL, "dc_roi_pixel_corr: without row_roi every CSR row is an ROI, but S = %d and R = %d", S, R);
  DC_REQUIRE((((uintptr_t)mom | (uintptr_t)rmom) & 7) == 0 &&
             (((uintptr_t)row_off | (uintptr_t)row_roi | (uintptr_t)inside | (uintptr_t)corr) & 3) == 0, DC_EINVAL,
             "dc_roi_pixel_corr: misaligned buffer");
  DC_REQUIRE(T <= DC_ROI_PIXEL_MAX_FRAMES, DC_EUNSUP, "dc_roi_pixel_corr: T = %ld: T is limited to 2^31 - 1 = %ld", T,
             (long)DC_ROI_PIXEL_MAX_FRAMES);
  if (N == 0 || S == 0) return DC_OK;
  hipLaunchKernelGGL(roi_pixel_corr_kernel, dim3((unsigned)S), dim3(kThreads), 0, (hipStream_t)stream, (const int64_t*)mom, (long)N, row_off,
                     row_roi, R, inside, (const int64_t*)rmom, (int64_t)T, corr);
  DC_CHECK_LAUNCH("dc_roi_pixel_corr");
  return DC_OK;
}
