// ROI fluorescence traces on the device: a recording (T, H, W) of 16-bit frames and a set of ROIs (pixel lists) -> one trace per
// ROI, the `traces` matrix (no. ROIs, no. frames) the reference's spikes model consumes (unet_1d_segmentation.py:182-187) and
// the per-trace normalisation (traces - mean) / std it applies along time (unet_1d_segmentation.py:158-167).
//
// Everything that can be exact is exact: a trace is the integer sum of the ROI's pixels in each frame (int64; int32 only inside
// one staged piece of a pixel list, where the bound below holds), the z-score numerators are formed in 128-bit integers
// (series_math.h) and rounded to double once.  Nothing in this file may be contracted into a fused multiply-add or reassociated:
// the pragma below and the per-file flag in _build.py.
#pragma clang fp contract(off)
#include <type_traits>

#include "common.h"
#include "series_math.h"
#include "wtrace_math.h"

namespace {

const int kThreads = 256;
const int kWave = 64;
const int kWaves = kThreads / kWave;
const int kFpw = 8;                   // frames a wave carries through one pass over the pixel list
const int kTile = kWaves * kFpw;      // frames per workgroup
const int kPiece = 2048;              // pixel indices staged in LDS at a time: 2048 * 65535 < 2^27, so int32 holds a piece's sum
const int kZeroBlocks = 1024;

template <bool UNS>
__device__ __forceinline__ int widen(uint16_t v) { return UNS ? (int)v : (int)(int16_t)v; }

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// the weighted form: not one term w x fits int32 (wtrace_math.h), so the lanes' partial sums and their reduction are 64 bits wide
__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// columns [t0, t0 + tc) of all R rows <- 0: what the atomic form of the accumulate kernel adds into
__global__ __launch_bounds__(kThreads) void roi_trace_zero_kernel(int64_t* __restrict__ sums, long ld, long t0, int tc, int R) {
  const long n = (long)R * tc;
  for (long i = (long)blockIdx.x * kThreads + threadIdx.x; i < n; i += (long)gridDim.x * kThreads)
    sums[(i / tc) * ld + t0 + (i % tc)] = 0;
}

// One workgroup per (CSR row, tile of kTile frames).  The row's pixel indices sit in LDS (sanitised: an index outside the image
// becomes -1 and is never dereferenced) while every wave gathers them from its kFpw frames -- kFpw independent 2-byte loads per
// index in flight per lane --, sums in int32, reduces across the wave and adds the piece into its int64 totals.  One value per
// (row, frame) leaves the workgroup: a plain store when rows are ROIs (row_roi == null), an integer atomic into the column the
// same call has zeroed when several rows share an ROI (integer addition: the order does not matter).
// WGT (dc_roi_wtrace_accumulate): every entry carries a 16-bit weight, staged beside its index; a term is w x, formed and summed in
// int64 (wtrace_math.h derives why no 32-bit partial survives a weight).  Without WGT nothing differs: no weights in LDS, int32
// partial sums within a piece.
template <bool UNS, bool WGT>
__global__ __launch_bounds__(kThreads) void roi_trace_accumulate_kernel(const uint16_t* __restrict__ frames, int tc, long t0,
                                                                       const int* __restrict__ row_off, const int* __restrict__ row_pix,
                                                                       const uint16_t* __restrict__ row_wgt, const int* __restrict__ row_roi,
                                                                       int R, int64_t* __restrict__ sums, long ld, long HW, int tiles) {
  typedef typename std::conditional<WGT, int64_t, int>::type part_t;
  __shared__ int pix[kPiece];
  __shared__ uint16_t wgt[WGT ? kPiece : 1];
  const int s = blockIdx.x, wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const long a = row_off[s], b = row_off[s + 1];
  const int r = row_roi ? row_roi[s] : s;
  if (r < 0 || r >= R) return;                       // the whole workgroup: a row that names no ROI adds nowhere
  for (int tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
    const int f0 = tile * kTile + wave * kFpw;       // this wave's first frame within the chunk
    const int nf = tc - f0 < kFpw ? tc - f0 : kFpw;  // <= 0: the wave only helps staging
    const uint16_t* f = frames + (long)f0 * HW;
    int64_t acc[kFpw];
#pragma unroll
    for (int k = 0; k < kFpw; ++k) acc[k] = 0;
    for (long p0 = a; p0 < b; p0 += kPiece) {
      const int m = (int)(b - p0 < kPiece ? b - p0 : kPiece);
      __syncthreads();                               // the readers of the previous piece are done
      for (int i = threadIdx.x; i < m; i += kThreads) {
        const int q = row_pix[p0 + i];
        pix[i] = (q >= 0 && q < HW) ? q : -1;
        if (WGT) wgt[i] = row_wgt[p0 + i];
      }
      __syncthreads();
      part_t v[kFpw];
#pragma unroll
      for (int k = 0; k < kFpw; ++k) v[k] = 0;
      for (int i = lane; i < m; i += kWave) {
        const int q = pix[i];
        if (q < 0) continue;
        if (WGT) {
          const int w = wgt[i];
#pragma unroll
          for (int k = 0; k < kFpw; ++k)
            if (k < nf) v[k] += dc_wtrace_term(w, widen<UNS>(f[(long)k * HW + q]));
        } else {
#pragma unroll
          for (int k = 0; k < kFpw; ++k)
            if (k < nf) v[k] += widen<UNS>(f[(long)k * HW + q]);
        }
      }
#pragma unroll
      for (int k = 0; k < kFpw; ++k) acc[k] += wave_sum(v[k]);
    }
    int64_t* out = sums + (long)r * ld + t0 + f0;
#pragma unroll
    for (int k = 0; k < kFpw; ++k)
      if (lane == k && k < nf) {
        if (row_roi) atomicAdd(reinterpret_cast<unsigned long long*>(out + k), (unsigned long long)acc[k]);
        else out[k] = acc[k];
      }
  }
}

// sums -> float32 traces, one workgroup per ROI.  With S_t the ROI's sum in frame t, the area cancels out of the z-score:
// z_t = (T S_t - sum S) / sqrt(T sum S^2 - (sum S)^2).  sum S^2 exceeds 64 bits (a whole-image ROI of a 260 x 256 uint16 frame:
// S^2 > 2^64); with T * H * W <= 2^46 every intermediate stays below 2^124.
__global__ __launch_bounds__(kThreads) void roi_trace_finalize_kernel(const int64_t* __restrict__ sums, long ld, const int* __restrict__ areas,
                                                                     int64_t T, float* __restrict__ mean, float* __restrict__ zscore) {
  __shared__ int64_t sm1[kThreads];
  __shared__ uint64_t sm2lo[kThreads];
  __shared__ int64_t sm2hi[kThreads];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int64_t* row = sums + (long)r * ld;
  const int area = areas[r];
  if (area <= 0) {                                   // no pixels: no trace
    for (int64_t t = tid; t < T; t += kThreads) {
      if (mean) mean[(long)r * T + t] = 0.f;
      if (zscore) zscore[(long)r * T + t] = 0.f;
    }
    return;
  }
  int64_t s1 = 0;
  DcI128 den = {0, 0};
  if (zscore) {
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
    s1 = sm1[0];
    s2.lo = sm2lo[0]; s2.hi = sm2hi[0];
    den = dc_i128_sub(dc_i128_mul_i64(s2, T), dc_i128_mul(s1, s1));       // exact, >= 0
  }
  const bool flat = dc_i128_is_zero(den);            // constant in time (T == 1 included): exactly 0, where numpy gives NaN
  const double root = flat ? 1.0 : sqrt(dc_i128_to_f64(den));
  const double ad = (double)area;
  for (int64_t t = tid; t < T; t += kThreads) {
    const int64_t v = row[t];
    if (mean) mean[(long)r * T + t] = (float)((double)v / ad);
    if (zscore) {
      const DcI128 num = dc_i128_sub(dc_i128_mul(T, v), dc_i128_from_i64(s1));
      zscore[(long)r * T + t] = flat ? 0.f : (float)(dc_i128_to_f64(num) / root);
    }
  }
}

}  // namespace

// the two accumulate entry points: one set of checks and one launch, row_wgt == null for the unweighted one
static int roi_accumulate(const char* who, bool weighted, const void* frames, int is_unsigned, int tc, long t0, const int* row_off,
                          const int* row_pix, const unsigned short* row_wgt, const int* row_roi, int S, int R, long* sums, long ld, int H, int W,
                          dc_stream_t stream) {
  DC_REQUIRE(frames && row_off && row_pix && sums && (row_wgt || !weighted), DC_EINVAL, "%s: null pointer", who);
  DC_REQUIRE(S >= 0 && R >= 0 && tc >= 0 && t0 >= 0, DC_EINVAL, "%s: negative count (S %d, R %d, tc %d, t0 %ld)", who, S, R, tc, t0);
  DC_REQUIRE_FRAMES(who, tc);
  DC_REQUIRE(row_roi || S == R, DC_EINVAL, "%s: without row_roi every CSR row is an ROI, but S = %d and R = %d", who, S, R);
  DC_REQUIRE(ld >= t0 + tc, DC_EINVAL, "%s: ld = %ld is below t0 + tc = %ld", who, ld, t0 + tc);
  DC_REQUIRE(H > 0 && W > 0 && (long)H * W <= (1L << 30), DC_EINVAL, "%s: image %d x %d out of range", who, H, W);
  DC_REQUIRE(((((uintptr_t)frames) | (uintptr_t)row_wgt) & 1) == 0 && (((uintptr_t)row_off | (uintptr_t)row_pix | (uintptr_t)row_roi) & 3) == 0 &&
             (((uintptr_t)sums) & 7) == 0, DC_EINVAL, "%s: misaligned buffer", who);
  const long HW = (long)H * W;
  DC_REQUIRE(t0 + tc <= DC_ROI_TRACE_MAX_VOLUME / HW, DC_EUNSUP, "%s: %ld frames of %d x %d: T * H * W is limited to 2^46 = %ld", who, t0 + tc, H, W,
             (long)DC_ROI_TRACE_MAX_VOLUME);
  if (R == 0 || tc == 0) return DC_OK;
  int64_t* out = (int64_t*)sums;
  if (row_roi) {
    const long n = (long)R * tc;
    const int blocks = (int)(dc_cdiv(n, kThreads) < kZeroBlocks ? dc_cdiv(n, kThreads) : kZeroBlocks);
    hipLaunchKernelGGL(roi_trace_zero_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, out, ld, t0, tc, R);
    char zero_name[64];
    snprintf(zero_name, sizeof zero_name, "%s(zero)", who);
    DC_CHECK_LAUNCH(zero_name);
    if (S == 0) return DC_OK;
  }
  const int tiles = dc_cdiv(tc, kTile);
  const dim3 grid((unsigned)S, (unsigned)(tiles < 65535 ? tiles : 65535)), block(kThreads);
  const uint16_t* f = (const uint16_t*)frames;
  const uint16_t* w = (const uint16_t*)row_wgt;
#define DC_ROI_ACC(UNS, WGT)                                                                                                              \
  hipLaunchKernelGGL((roi_trace_accumulate_kernel<UNS, WGT>), grid, block, 0, (hipStream_t)stream, f, tc, t0, row_off, row_pix, w, row_roi, R, \
                     out, ld, HW, tiles)
  if (weighted) {
    if (is_unsigned) DC_ROI_ACC(true, true);
    else DC_ROI_ACC(false, true);
  } else {
    if (is_unsigned) DC_ROI_ACC(true, false);
    else DC_ROI_ACC(false, false);
  }
#undef DC_ROI_ACC
  DC_CHECK_LAUNCH(who);
  return DC_OK;
}

extern "C" int dc_roi_trace_accumulate(const void* frames, int is_unsigned, int tc, long t0, const int* row_off, const int* row_pix,
                                       const int* row_roi, int S, int R, long* sums, long ld, int H, int W, dc_stream_t stream) {
  return roi_accumulate("dc_roi_trace_accumulate", false, frames, is_unsigned, tc, t0, row_off, row_pix, nullptr, row_roi, S, R, sums, ld, H, W,
                        stream);
}

extern "C" int dc_roi_wtrace_accumulate(const void* frames, int is_unsigned, int tc, long t0, const int* row_off, const int* row_pix,
                                        const unsigned short* row_wgt, const int* row_roi, int S, int R, long* sums, long ld, int H, int W,
                                        dc_stream_t stream) {
  return roi_accumulate("dc_roi_wtrace_accumulate", true, frames, is_unsigned, tc, t0, row_off, row_pix, row_wgt, row_roi, S, R, sums, ld, H, W,
                        stream);
}

extern "C" int dc_roi_trace_finalize(const long* sums, long ld, const int* areas, int R, long T, float* mean, float* zscore,
                                     dc_stream_t stream) {
  DC_REQUIRE(sums && areas, DC_EINVAL, "dc_roi_trace_finalize: null pointer");
  DC_REQUIRE(R >= 0 && T >= 0, DC_EINVAL, "dc_roi_trace_finalize: negative count (R %d, T %ld)", R, T);
  DC_REQUIRE(ld >= T, DC_EINVAL, "dc_roi_trace_finalize: ld = %ld is below T = %ld", ld, T);
  DC_REQUIRE((((uintptr_t)sums) & 7) == 0 && (((uintptr_t)areas | (uintptr_t)mean | (uintptr_t)zscore) & 3) == 0, DC_EINVAL,
             "dc_roi_trace_finalize: misaligned buffer");
  DC_REQUIRE(T <= DC_ROI_TRACE_MAX_VOLUME, DC_EUNSUP, "dc_roi_trace_finalize: T = %ld: T * H * W is limited to 2^46 = %ld", T,
             (long)DC_ROI_TRACE_MAX_VOLUME);
  if (R == 0 || T == 0 || (!mean && !zscore)) return DC_OK;
  hipLaunchKernelGGL(roi_trace_finalize_kernel, dim3((unsigned)R), dim3(kThreads), 0, (hipStream_t)stream, (const int64_t*)sums, ld, areas,
                     (int64_t)T, mean, zscore);
  DC_CHECK_LAUNCH("dc_roi_trace_finalize");
  return DC_OK;
}
