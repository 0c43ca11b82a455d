// Series summaries on the device: the (H, W) images a recording (T, H, W) of 16-bit frames is reduced to before segmentation --
// the reference's stored float16 mean and int16 max (datasets/nf.py:121-130), the true mean, max and temporal standard deviation,
// the local correlation image, and the image standardisation of _summarize_series (unet_2d_summary.py:227-241) -- and, in front of
// every reader of a recording, the temporal bins: the exact rounded means of b consecutive frames (dc_series_bin_time).
//
// Everything that can be exact is exact: the running sums are integers, the variance / covariance numerators are formed in 128-bit
// integer arithmetic (series_math.h), and the float16 chain rounds once per frame from an IEEE double, as numpy does.  Nothing in
// this file may be contracted into a fused multiply-add or reassociated: the pragma below and the per-file flag in _build.py.
#pragma clang fp contract(off)
#include "common.h"
#include "series_math.h"
#include "detrend_math.h"

namespace {

const int kPix = 4;                   // pixels per lane: one 8-byte load per frame
const int kThreads = 256;
const int kStdBlocks = 64;            // partial rows of dc_image_standardize

// frames carry no alignment beyond their element size: H * W may be odd, so frame t starts at any even byte offset
typedef uint16_t u16x4_any __attribute__((ext_vector_type(4), aligned(2)));

template <bool UNS>
__device__ __forceinline__ int widen(uint16_t v) { return UNS ? (int)v : (int)(int16_t)v; }

// pixels [p, p + 4) of one frame; elements at or beyond `n` valid ones read as 0
template <bool UNS>
__device__ __forceinline__ void load4(const uint16_t* __restrict__ f, int n, int (&v)[kPix]) {
  if (n >= kPix) {
    const u16x4_any r = *reinterpret_cast<const u16x4_any*>(f);
    v[0] = widen<UNS>(r.x); v[1] = widen<UNS>(r.y); v[2] = widen<UNS>(r.z); v[3] = widen<UNS>(r.w);
  } else {
#pragma unroll
    for (int k = 0; k < kPix; ++k) v[k] = k < n ? widen<UNS>(f[k]) : 0;
  }
}

// ---- one streaming pass: exact integer sums, true max, and the reference's float16 mean / saturated int16 max chains ----------
// A lane owns 4 consecutive pixels of the flattened image for all tc frames of the chunk (the float16 chain is sequential in t by
// definition; the integers just ride along), state in registers, read and written once per chunk.
template <bool UNS, bool CHAIN>
__global__ __launch_bounds__(kThreads) void series_accumulate_kernel(const uint16_t* __restrict__ frames, int tc, int first,
                                                                    double n_total, uint16_t* __restrict__ mean16,
                                                                    int16_t* __restrict__ max16, int64_t* __restrict__ sum,
                                                                    int64_t* __restrict__ sumsq, int* __restrict__ vmax, long HW) {
  const long p0 = ((long)blockIdx.x * kThreads + threadIdx.x) * kPix;
  if (p0 >= HW) return;
  const int n = (int)(HW - p0 < kPix ? HW - p0 : kPix);
  int64_t s[kPix], ss[kPix];
  int vm[kPix], m16[kPix];
  double m[kPix];
#pragma unroll
  for (int k = 0; k < kPix; ++k) {
    const bool live = k < n && !first;
    s[k] = live ? sum[p0 + k] : 0;
    ss[k] = live ? sumsq[p0 + k] : 0;
    vm[k] = live ? vmax[p0 + k] : INT32_MIN;
    m[k] = (CHAIN && live) ? dc_f16_bits_to_f64(mean16[p0 + k]) : 0.0;
    m16[k] = (CHAIN && live) ? (int)max16[p0 + k] : 0;
  }
  const uint16_t* f = frames + p0;
#pragma unroll 4
  for (int t = 0; t < tc; ++t) {
    int v[kPix];
    load4<UNS>(f + (long)t * HW, n, v);
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
      const int x = v[k];
      s[k] += x;
      ss[k] += (int64_t)x * (int64_t)x;
      vm[k] = x > vm[k] ? x : vm[k];
      if (CHAIN) {
        // nf.py:129  ds_mean[...] += img * 1. / n : double divide, double add, ONE rounding to the float16 storage
        m[k] = dc_f16_bits_to_f64(dc_f64_to_f16_bits(m[k] + (double)x / n_total));
        // nf.py:130  np.maximum(ds_max, img) stored as int16: the conversion on store saturates
        const int mx = x > m16[k] ? x : m16[k];
        m16[k] = mx > 32767 ? 32767 : mx;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kPix; ++k)
    if (k < n) {
      sum[p0 + k] = s[k];
      sumsq[p0 + k] = ss[k];
      vmax[p0 + k] = vm[k];
      if (CHAIN) {
        mean16[p0 + k] = dc_f64_to_f16_bits(m[k]);
        max16[p0 + k] = (int16_t)m16[k];
      }
    }
}

// ---- cross sums with the four forward neighbours ------------------------------------------------------------------------
// A lane owns 4 consecutive pixels of ONE row; per frame it reads that row at [x0, x0 + 5) and the row below at [x0 - 1, x0 + 5)
// (its neighbours' values come out of the cache: HBM sees every frame once).  A value outside the image is 0, so its products
// contribute nothing.  xy = int64[4][H * W]: right, down, down-right, down-left.
template <bool UNS>
__global__ __launch_bounds__(kThreads) void series_accumulate_xy_kernel(const uint16_t* __restrict__ frames, int tc, int first,
                                                                       int64_t* __restrict__ xy, int H, int W, int groups) {
  const long idx = (long)blockIdx.x * kThreads + threadIdx.x;
  const int y = (int)(idx / groups), x0 = (int)(idx % groups) * kPix;
  if (y >= H) return;
  const long HW = (long)H * W, p0 = (long)y * W + x0;
  const int n = W - x0 < kPix ? W - x0 : kPix;
  const bool below = y + 1 < H, left = x0 > 0, right = x0 + kPix < W;
  int64_t a[4][kPix];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < kPix; ++k) a[j][k] = (k < n && !first) ? xy[j * HW + p0 + k] : 0;
  const uint16_t* f = frames + p0;
#pragma unroll 4
  for (int t = 0; t < tc; ++t) {
    const uint16_t* ft = f + (long)t * HW;
    int c[kPix + 1], d[kPix + 2] = {0, 0, 0, 0, 0, 0};      // c[k] = row y at x0 + k ; d[k] = row y + 1 at x0 - 1 + k
    int v[kPix];
    load4<UNS>(ft, n, v);
#pragma unroll
    for (int k = 0; k < kPix; ++k) c[k] = v[k];
    c[kPix] = right ? widen<UNS>(ft[kPix]) : 0;
    if (below) {
      load4<UNS>(ft + W, n, v);
#pragma unroll
      for (int k = 0; k < kPix; ++k) d[k + 1] = v[k];
      d[0] = left ? widen<UNS>(ft[W - 1]) : 0;
      d[kPix + 1] = right ? widen<UNS>(ft[W + kPix]) : 0;
    }
#pragma unroll
    for (int k = 0; k < kPix; ++k) {
      const int64_t x = c[k];
      a[0][k] += x * (int64_t)c[k + 1];
      a[1][k] += x * (int64_t)d[k + 1];
      a[2][k] += x * (int64_t)d[k + 2];
      a[3][k] += x * (int64_t)d[k];
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int k = 0; k < kPix; ++k)
      if (k < n) xy[j * HW + p0 + k] = a[j][k];
}

// ---- state -> float32 images ----------------------------------------------------------------------------------------------
// T * sum(x^2) - sum(x)^2 reaches 2^94 and T * sum(xy) - sum(x) sum(y) as much: formed exactly, then ONE conversion to double.
__device__ __forceinline__ DcI128 central2(int64_t T, int64_t sxy, int64_t sx, int64_t sy) {
  return dc_i128_sub(dc_i128_mul(T, sxy), dc_i128_mul(sx, sy));
}

__global__ __launch_bounds__(kThreads) void series_finalize_kernel(const int64_t* __restrict__ sum, const int64_t* __restrict__ sumsq,
                                                                  const int64_t* __restrict__ xy, float* __restrict__ mean,
                                                                  float* __restrict__ sd, float* __restrict__ corr, int H, int W,
                                                                  int64_t T) {
  const long HW = (long)H * W, p = (long)blockIdx.x * kThreads + threadIdx.x;
  if (p >= HW) return;
  const int y = (int)(p / W), x = (int)(p % W);
  const int64_t sx = sum[p];
  const DcI128 vp = central2(T, sumsq[p], sx, sx);
  const double Td = (double)T;
  if (mean) mean[p] = (float)((double)sx / Td);
  if (sd) sd[p] = (float)(sqrt(dc_i128_to_f64(vp)) / Td);
  if (!corr) return;
  const double vpd = dc_i128_to_f64(vp);
  const bool flat = dc_i128_is_zero(vp);
  double acc = 0.0;
  int cnt = 0;
  // the pair (p, q) is stored with the EARLIER pixel in raster order: slot 0 right, 1 down, 2 down-right, 3 down-left
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int dy = j < 3 ? -1 : (j < 5 ? 0 : 1);
    const int dx = j < 3 ? j - 1 : (j == 3 ? -1 : (j == 4 ? 1 : j - 6));
    const int qy = y + dy, qx = x + dx;
    if (qy < 0 || qy >= H || qx < 0 || qx >= W) continue;
    ++cnt;
    if (flat) continue;
    const long q = (long)qy * W + qx;
    const int64_t sy = sum[q];
    const DcI128 vq = central2(T, sumsq[q], sy, sy);
    if (dc_i128_is_zero(vq)) continue;
    const int slot = dy == 0 ? 0 : (dx == 0 ? 1 : (dx == dy ? 2 : 3));
    const long owner = (dy > 0 || (dy == 0 && dx > 0)) ? p : q;
    const DcI128 num = central2(T, xy[slot * HW + owner], sx, sy);
    acc += dc_i128_to_f64(num) / sqrt(vpd * dc_i128_to_f64(vq));
  }
  corr[p] = cnt ? (float)(acc / (double)cnt) : 0.f;
}

// ---- detrended summaries: segment-pooled centred moments (the definitions are in include/dcunet.h, "Detrended correlations") ----------
// At the end of a segment of `len` frames the segment's sums are folded into the pooled numerators: one lane per pixel, which
// alone owns the pixel's pooled words (variance, the four pairs it is the EARLIER pixel of, total sum and maximum).  The
// neighbours' segment sums are only read, and nothing of the segment state is written: the next segment's first accumulate
// (t0 == 0) initialises it.  A neighbour outside the image contributes nothing: its slot stays 0.
__global__ __launch_bounds__(kThreads) void series_fold_segment_kernel(const int64_t* __restrict__ sum, const int64_t* __restrict__ sumsq,
                                                                      const int64_t* __restrict__ xy, const int* __restrict__ vmax,
                                                                      int64_t len, int64_t mult, int64_t* __restrict__ pvar,
                                                                      int64_t* __restrict__ pcov, int64_t* __restrict__ sum_total,
                                                                      int* __restrict__ vmax_total, int H, int W) {
  const long HW = (long)H * W, p = (long)blockIdx.x * kThreads + threadIdx.x;
  if (p >= HW) return;
  const int y = (int)(p / W), x = (int)(p % W);
  const int64_t sx = sum[p];
  dc_i128_store(pvar, p, dc_i128_add(dc_i128_load(pvar, p), dc_detrend_term(len, mult, sumsq[p], sx, sx)));
  sum_total[p] += sx;
  const int vm = vmax[p], vt = vmax_total[p];
  vmax_total[p] = vm > vt ? vm : vt;
  if (!xy) return;
#pragma unroll
  for (int j = 0; j < 4; ++j) {                      // slot 0 right, 1 down, 2 down-right, 3 down-left
    const int qy = y + (j > 0), qx = x + (j == 0 || j == 2) - (j == 3);
    if (qy >= H || qx < 0 || qx >= W) continue;
    const long q = (long)qy * W + qx, e = j * HW + p;
    dc_i128_store(pcov, e, dc_i128_add(dc_i128_load(pcov, e), dc_detrend_term(len, mult, xy[e], sx, sum[q])));
  }
}

// pooled numerators -> float32 images: the neighbour rule and the summation order of series_finalize_kernel, the numerators read
// instead of formed
__global__ __launch_bounds__(kThreads) void series_finalize_pooled_kernel(const int64_t* __restrict__ pvar, const int64_t* __restrict__ pcov,
                                                                         const int64_t* __restrict__ sum_total, float* __restrict__ mean,
                                                                         float* __restrict__ sd, float* __restrict__ corr, int H, int W,
                                                                         int64_t M, int64_t T) {
  const long HW = (long)H * W, p = (long)blockIdx.x * kThreads + threadIdx.x;
  if (p >= HW) return;
  const int y = (int)(p / W), x = (int)(p % W);
  const DcI128 vp = dc_i128_load(pvar, p);
  if (mean) mean[p] = (float)((double)sum_total[p] / (double)T);
  if (sd) sd[p] = (float)sqrt(dc_detrend_var(vp, M, T));
  if (!corr) return;
  const double vpd = dc_i128_to_f64(vp);
  const bool flat = !dc_i128_is_positive(vp);
  double acc = 0.0;
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int dy = j < 3 ? -1 : (j < 5 ? 0 : 1);
    const int dx = j < 3 ? j - 1 : (j == 3 ? -1 : (j == 4 ? 1 : j - 6));
    const int qy = y + dy, qx = x + dx;
    if (qy < 0 || qy >= H || qx < 0 || qx >= W) continue;
    ++cnt;
    if (flat) continue;
    const long q = (long)qy * W + qx;
    const DcI128 vq = dc_i128_load(pvar, q);
    if (!dc_i128_is_positive(vq)) continue;
    const int slot = dy == 0 ? 0 : (dx == 0 ? 1 : (dx == dy ? 2 : 3));
    const long owner = (dy > 0 || (dy == 0 && dx > 0)) ? p : q;
    acc += dc_i128_to_f64(dc_i128_load(pcov, slot * HW + owner)) / sqrt(vpd * dc_i128_to_f64(vq));
  }
  corr[p] = cnt ? (float)(acc / (double)cnt) : 0.f;
}

// ---- (img - mean(img)) / std(img), unet_2d_summary.py:239 ------------------------------------------------------------------
// Three launches over one small image, every sum a fixed-order tree in double (the form of dc_reduce_partials_f64): per-block
// partial sums -> the mean; per-block partial sums of (v - mean)^2 -> the population standard deviation (two-pass, as numpy's
// std); the apply pass.  Each block re-derives mean / std from the same partial rows in the same order: identical values.
__device__ __forceinline__ double block_sum(double s, double* sm) {
  const int tid = threadIdx.x;
  sm[tid] = s;
  __syncthreads();
  for (int k = kThreads / 2; k > 0; k >>= 1) {
    if (tid < k) sm[tid] += sm[tid + k];
    __syncthreads();
  }
  const double r = sm[0];
  __syncthreads();
  return r;
}
__device__ __forceinline__ double rows_sum(const double* __restrict__ part, double* sm) {
  return block_sum(threadIdx.x < kStdBlocks ? part[threadIdx.x] : 0.0, sm);
}
template <int PASS>
__global__ __launch_bounds__(kThreads) void image_standardize_kernel(const float* in, float* out,      // may alias: in == out is allowed
                                                                   
                                                                    double* __restrict__ ws, long n) {
  __shared__ double sm[kThreads];
  const double cnt = (double)n;
  double mu = 0.0, sd = 0.0;
  if (PASS >= 1) mu = rows_sum(ws, sm) / cnt;
  if (PASS == 2) sd = sqrt(rows_sum(ws + kStdBlocks, sm) / cnt);
  const long per = (n + kStdBlocks - 1) / kStdBlocks, i0 = blockIdx.x * per, i1 = i0 + per < n ? i0 + per : n;
  double s = 0.0;
  for (long i = i0 + threadIdx.x; i < i1; i += kThreads) {
    const double v = (double)in[i];
    if (PASS == 0) s += v;
    if (PASS == 1) s += (v - mu) * (v - mu);
    if (PASS == 2) out[i] = (float)((v - mu) / sd);
  }
  if (PASS < 2) {
    s = block_sum(s, sm);
    if (threadIdx.x == 0) ws[PASS * kStdBlocks + blockIdx.x] = s;
  }
}

// ---- temporal binning: out[j] = the rounded mean of b consecutive frames (the definitions are in include/dcunet.h) ------------------
// One memory-bound pass that reads every input value once.  A work item is one output SLOT -- the n_out bins the call closes and,
// behind them, the bin it leaves open -- times one group of 8 consecutive pixels: blockIdx.y strides over the slots, the x grid
// over the groups, so a 64-frame chunk at b = 4 is 17 * H * W / 8 items and neighbouring lanes read neighbouring 16-byte pieces.
// Slot j holds the chunk's frames [j b - phase, (j + 1) b - phase) that exist; only slot 0 starts from `carry` (phase > 0), only
// the open slot writes it.  `carry` is updated in place, so where one call does both (phase > 0, a bin closed, a bin left open)
// the open slot is no item of its own: the item of slot 0 adds it up and stores it AFTER it has read the old carry of the same
// pixels (`ride`) -- an item of its own would race with that read.  16-byte loads and stores where every frame starts 16-byte
// aligned (H * W % 8 == 0 and an aligned base; in, out and carry each on their own), value by value otherwise -- a ragged last
// group included.
const int kBinPix = 8;                // pixels per item
const int kBinBlocksX = 4096;         // workgroups along the groups; the slots stride at 65535

// s[k] += pixel k of the frames [i0, i1) of the chunk, for the n valid pixels of the group at f0 = frames + p0
template <bool UNS>
__device__ __forceinline__ void bin_add_frames(const uint16_t* __restrict__ f0, int i0, int i1, int HW, int n, int wide_in, int (&s)[kBinPix]) {
  const uint16_t* f = f0 + (long)i0 * HW;
#pragma unroll 4
  for (int i = i0; i < i1; ++i, f += HW) {
    unsigned w[kBinPix / 2];
    if (wide_in) {                                       // H * W % 8 == 0: every group is whole
      const uint4 v = *reinterpret_cast<const uint4*>(f);
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
      for (int q = 0; q < kBinPix / 2; ++q) {
        const unsigned a = 2 * q < n ? f[2 * q] : 0u, c = 2 * q + 1 < n ? f[2 * q + 1] : 0u;
        w[q] = a | (c << 16);
      }
    }
#pragma unroll
    for (int k = 0; k < kBinPix; ++k) s[k] += widen<UNS>((uint16_t)((w[k / 2] >> (16 * (k & 1))) & 0xffffu));
  }
}

__device__ __forceinline__ void bin_put_carry(int* __restrict__ c, int n, int wide_carry, const int (&s)[kBinPix]) {
  if (wide_carry && n == kBinPix) {
    *reinterpret_cast<int4*>(c) = make_int4(s[0], s[1], s[2], s[3]);
    *reinterpret_cast<int4*>(c + 4) = make_int4(s[4], s[5], s[6], s[7]);
  } else {
#pragma unroll
    for (int k = 0; k < kBinPix; ++k)
      if (k < n) c[k] = s[k];
  }
}

// n_slots: the slots that are items of their own -- n_out, plus the open one unless it rides on slot 0
template <bool UNS>
__global__ __launch_bounds__(kThreads) void series_bin_time_kernel(const uint16_t* __restrict__ frames, int tc, int HW, int b, int phase,
                                                                  uint32_t magic, int* carry, uint16_t* __restrict__ out, int n_out,
                                                                  int n_slots, int ride, int wide_in, int wide_out, int wide_carry) {
  const int G = (HW + kBinPix - 1) / kBinPix;
  for (long j = blockIdx.y; j < n_slots; j += gridDim.y) {
    const long lo = j * b - phase;
    const int i0 = lo < 0 ? 0 : (int)lo, i1 = lo + b < tc ? (int)(lo + b) : tc;
    const bool head = j == 0 && phase > 0, open = j >= n_out;
    for (int g = blockIdx.x * kThreads + threadIdx.x; g < G; g += gridDim.x * kThreads) {
      const int p0 = g * kBinPix;
      const int n = HW - p0 < kBinPix ? HW - p0 : kBinPix;
      int s[kBinPix];
#pragma unroll
      for (int k = 0; k < kBinPix; ++k) s[k] = 0;
      if (head) {
        if (wide_carry && n == kBinPix) {
          const int4 c0 = *reinterpret_cast<const int4*>(carry + p0), c1 = *reinterpret_cast<const int4*>(carry + p0 + 4);
          s[0] = c0.x; s[1] = c0.y; s[2] = c0.z; s[3] = c0.w; s[4] = c1.x; s[5] = c1.y; s[6] = c1.z; s[7] = c1.w;
        } else {
#pragma unroll
          for (int k = 0; k < kBinPix; ++k)
            if (k < n) s[k] = carry[p0 + k];
        }
      }
      bin_add_frames<UNS>(frames + p0, i0, i1, HW, n, wide_in, s);
      if (open) {                                        // head and open at once: no bin closes, the thread's own read came first
        bin_put_carry(carry + p0, n, wide_carry, s);
        continue;
      }
      unsigned r[kBinPix];
#pragma unroll
      for (int k = 0; k < kBinPix; ++k) r[k] = (unsigned)dc_series_bin_round(s[k], b, magic) & 0xffffu;
      uint16_t* o = out + j * HW + p0;
      if (wide_out) {
        *reinterpret_cast<uint4*>(o) = make_uint4(r[0] | (r[1] << 16), r[2] | (r[3] << 16), r[4] | (r[5] << 16), r[6] | (r[7] << 16));
      } else {
#pragma unroll
        for (int k = 0; k < kBinPix; ++k)
          if (k < n) o[k] = (uint16_t)r[k];
      }
      if (head && ride) {                                // the open bin of these pixels: frames [n_out b - phase, tc)
#pragma unroll
        for (int k = 0; k < kBinPix; ++k) s[k] = 0;
        bin_add_frames<UNS>(frames + p0, (int)((long)n_out * b - phase), tc, HW, n, wide_in, s);
        bin_put_carry(carry + p0, n, wide_carry, s);
      }
    }
  }
}

int series_check(const char* fn, const void* frames, int tc, long t0, int H, int W) {
  DC_REQUIRE(frames, DC_EINVAL, "%s: null pointer", fn);
  DC_REQUIRE(H > 0 && W > 0 && (long)H * W <= (1L << 30), DC_EINVAL, "%s: image %d x %d out of range", fn, H, W);
  DC_REQUIRE(tc > 0 && t0 >= 0, DC_EINVAL, "%s: chunk of %d frames at frame %ld", fn, tc, t0);
  DC_REQUIRE_FRAMES(fn, tc);
  DC_REQUIRE((((uintptr_t)frames) & 1) == 0, DC_EINVAL, "%s: frames must be 2-byte aligned", fn);
  return DC_OK;
}

}  // namespace

extern "C" int dc_series_accumulate(const void* frames, int is_unsigned, int tc, long t0, long n_total, uint16_t* mean16,
                                    int16_t* max16, long* sum, long* sumsq, int* vmax, int H, int W, dc_stream_t stream) {
  const int rc = series_check("dc_series_accumulate", frames, tc, t0, H, W);
  if (rc != DC_OK) return rc;
  DC_REQUIRE(sum && sumsq && vmax, DC_EINVAL, "dc_series_accumulate: null pointer");
  DC_REQUIRE((mean16 == nullptr) == (max16 == nullptr), DC_EINVAL, "dc_series_accumulate: mean16 and max16 come as a pair");
  DC_REQUIRE(n_total <= DC_SERIES_MAX_FRAMES, DC_EUNSUP, "dc_series_accumulate: %ld frames, the int64 state holds at most %ld",
             n_total, (long)DC_SERIES_MAX_FRAMES);
  DC_REQUIRE(t0 + tc <= n_total, DC_EINVAL, "dc_series_accumulate: frames [%ld, %ld) of a recording of %ld", t0, t0 + tc, n_total);
  DC_REQUIRE((((uintptr_t)sum) & 7) == 0 && (((uintptr_t)sumsq) & 7) == 0 && (((uintptr_t)vmax) & 3) == 0 && (((uintptr_t)mean16) & 1) == 0 &&
             (((uintptr_t)max16) & 1) == 0, DC_EINVAL, "dc_series_accumulate: misaligned state buffer");
  const long HW = (long)H * W;
  const dim3 grid((unsigned)dc_cdiv(dc_cdiv(HW, kPix), kThreads)), block(kThreads);
  const uint16_t* f = (const uint16_t*)frames;
  const int first = t0 == 0;
  const double nt = (double)n_total;
  int64_t* s = (int64_t*)sum;
  int64_t* ss = (int64_t*)sumsq;
#define DC_SERIES_LAUNCH(U, C)                                                                                              \
  hipLaunchKernelGGL((series_accumulate_kernel<U, C>), grid, block, 0, (hipStream_t)stream, f, tc, first, nt, mean16, max16, \
                     s, ss, vmax, HW)
  if (is_unsigned) { if (mean16) DC_SERIES_LAUNCH(true, true); else DC_SERIES_LAUNCH(true, false); }
  else { if (mean16) DC_SERIES_LAUNCH(false, true); else DC_SERIES_LAUNCH(false, false); }
#undef DC_SERIES_LAUNCH
  DC_CHECK_LAUNCH("dc_series_accumulate");
  return DC_OK;
}

extern "C" int dc_series_accumulate_xy(const void* frames, int is_unsigned, int tc, long t0, long* xy, int H, int W,
                                       dc_stream_t stream) {
  const int rc = series_check("dc_series_accumulate_xy", frames, tc, t0, H, W);
  if (rc != DC_OK) return rc;
  DC_REQUIRE(xy && (((uintptr_t)xy) & 7) == 0, DC_EINVAL, "dc_series_accumulate_xy: null or misaligned state buffer");
  const int groups = dc_cdiv(W, kPix);
  const dim3 grid((unsigned)dc_cdiv((long)H * groups, kThreads)), block(kThreads);
  const uint16_t* f = (const uint16_t*)frames;
  const int first = t0 == 0;
  if (is_unsigned)
    hipLaunchKernelGGL((series_accumulate_xy_kernel<true>), grid, block, 0, (hipStream_t)stream, f, tc, first, (int64_t*)xy, H, W, groups);
  else
    hipLaunchKernelGGL((series_accumulate_xy_kernel<false>), grid, block, 0, (hipStream_t)stream, f, tc, first, (int64_t*)xy, H, W, groups);
  DC_CHECK_LAUNCH("dc_series_accumulate_xy");
  return DC_OK;
}

extern "C" int dc_series_finalize(const long* sum, const long* sumsq, const long* xy, float* mean, float* sdev, float* corr,
                                  int H, int W, long T, dc_stream_t stream) {
  DC_REQUIRE(sum && sumsq && (((uintptr_t)sum | (uintptr_t)sumsq | (uintptr_t)xy) & 7) == 0, DC_EINVAL,
             "dc_series_finalize: null or misaligned state buffer");
  DC_REQUIRE(H > 0 && W > 0 && (long)H * W <= (1L << 30), DC_EINVAL, "dc_series_finalize: image %d x %d out of range", H, W);
  DC_REQUIRE(T > 0, DC_EINVAL, "dc_series_finalize: T = %ld", T);
  DC_REQUIRE(T <= DC_SERIES_MAX_FRAMES, DC_EUNSUP, "dc_series_finalize: T = %ld, the int64 state holds at most %ld frames", T,
             (long)DC_SERIES_MAX_FRAMES);
  DC_REQUIRE(corr == nullptr || xy != nullptr, DC_EINVAL, "dc_series_finalize: corr needs the xy state");
  hipLaunchKernelGGL(series_finalize_kernel, dim3((unsigned)dc_cdiv((long)H * W, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                     (const int64_t*)sum, (const int64_t*)sumsq, (const int64_t*)xy, mean, sdev, corr, H, W, (int64_t)T);
  DC_CHECK_LAUNCH("dc_series_finalize");
  return DC_OK;
}

extern "C" int dc_series_fold_segment(const long* sum, const long* sumsq, const long* xy, const int* vmax, long len, long mult,
                                      long* pooled_var, long* pooled_cov, long* sum_total, int* vmax_total, int H, int W,
                                      dc_stream_t stream) {
  DC_REQUIRE(sum && sumsq && vmax && pooled_var && sum_total && vmax_total, DC_EINVAL, "dc_series_fold_segment: null pointer");
  DC_REQUIRE((xy == nullptr) == (pooled_cov == nullptr), DC_EINVAL, "dc_series_fold_segment: xy and pooled_cov come as a pair");
  DC_REQUIRE((((uintptr_t)sum | (uintptr_t)sumsq | (uintptr_t)xy | (uintptr_t)sum_total) & 7) == 0 &&
             (((uintptr_t)vmax | (uintptr_t)vmax_total) & 3) == 0 && dc_aligned16(pooled_var) && dc_aligned16(pooled_cov), DC_EINVAL,
             "dc_series_fold_segment: misaligned state buffer (the pooled words are 16-byte elements)");
  DC_REQUIRE(H > 0 && W > 0 && (long)H * W <= (1L << 30), DC_EINVAL, "dc_series_fold_segment: image %d x %d out of range", H, W);
  DC_REQUIRE(len >= 1 && mult >= 1, DC_EINVAL, "dc_series_fold_segment: a segment of %ld frames with mult %ld", len, mult);
  DC_REQUIRE(dc_detrend_segment_ok(len, mult), DC_EUNSUP,
             "dc_series_fold_segment: len = %ld, mult = %ld: a segment beside others is limited to %d frames, one alone to %ld", len, mult,
             DC_DETREND_MAX_SEGMENT, (long)DC_SERIES_MAX_FRAMES);
  DC_REQUIRE(dc_detrend_volume_ok(len, mult, (long)H * W), DC_EUNSUP, "dc_series_fold_segment: M = %ld on %d x %d: M * H * W is limited to 2^46",
             len * mult, H, W);
  hipLaunchKernelGGL(series_fold_segment_kernel, dim3((unsigned)dc_cdiv((long)H * W, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                     (const int64_t*)sum, (const int64_t*)sumsq, (const int64_t*)xy, vmax, (int64_t)len, (int64_t)mult, (int64_t*)pooled_var,
                     (int64_t*)pooled_cov, (int64_t*)sum_total, vmax_total, H, W);
  DC_CHECK_LAUNCH("dc_series_fold_segment");
  return DC_OK;
}

extern "C" int dc_series_finalize_pooled(const long* pooled_var, const long* pooled_cov, const long* sum_total, float* mean, float* sdev,
                                         float* corr, int H, int W, long M, long T, dc_stream_t stream) {
  DC_REQUIRE(pooled_var && dc_aligned16(pooled_var) && dc_aligned16(pooled_cov) && (((uintptr_t)sum_total) & 7) == 0, DC_EINVAL,
             "dc_series_finalize_pooled: null or misaligned state buffer (the pooled words are 16-byte elements)");
  DC_REQUIRE((((uintptr_t)mean | (uintptr_t)sdev | (uintptr_t)corr) & 3) == 0, DC_EINVAL, "dc_series_finalize_pooled: misaligned image");
  DC_REQUIRE(H > 0 && W > 0 && (long)H * W <= (1L << 30), DC_EINVAL, "dc_series_finalize_pooled: image %d x %d out of range", H, W);
  DC_REQUIRE(T > 0 && M > 0, DC_EINVAL, "dc_series_finalize_pooled: M = %ld, T = %ld", M, T);
  DC_REQUIRE(T <= DC_SERIES_MAX_FRAMES && M <= DC_SERIES_MAX_FRAMES, DC_EUNSUP,
             "dc_series_finalize_pooled: M = %ld, T = %ld: each is limited to %ld", M, T, (long)DC_SERIES_MAX_FRAMES);
  DC_REQUIRE(dc_detrend_volume_ok(M, 1, (long)H * W), DC_EUNSUP, "dc_series_finalize_pooled: M = %ld on %d x %d: M * H * W is limited to 2^46",
             M, H, W);
  DC_REQUIRE(corr == nullptr || pooled_cov != nullptr, DC_EINVAL, "dc_series_finalize_pooled: corr needs the pooled_cov state");
  DC_REQUIRE(mean == nullptr || sum_total != nullptr, DC_EINVAL, "dc_series_finalize_pooled: mean needs the sum_total state");
  hipLaunchKernelGGL(series_finalize_pooled_kernel, dim3((unsigned)dc_cdiv((long)H * W, kThreads)), dim3(kThreads), 0, (hipStream_t)stream,
                     (const int64_t*)pooled_var, (const int64_t*)pooled_cov, (const int64_t*)sum_total, mean, sdev, corr, H, W, (int64_t)M,
                     (int64_t)T);
  DC_CHECK_LAUNCH("dc_series_finalize_pooled");
  return DC_OK;
}

extern "C" int dc_series_bin_time(const void* frames, int is_unsigned, int tc, int H, int W, int b, int phase, int* carry, void* out,
                                  dc_stream_t stream) {
  DC_REQUIRE(b >= 1, DC_EINVAL, "dc_series_bin_time: b = %d: a bin holds at least one frame", b);
  DC_REQUIRE(b <= DC_SERIES_MAX_BIN_FRAMES, DC_EUNSUP, "dc_series_bin_time: b = %d: a bin is limited to %d frames", b, DC_SERIES_MAX_BIN_FRAMES);
  DC_REQUIRE(phase >= 0 && phase < b, DC_EINVAL, "dc_series_bin_time: phase = %d outside [0, %d)", phase, b);
  DC_REQUIRE(tc >= 0 && H > 0 && W > 0, DC_EINVAL, "dc_series_bin_time: negative or zero size (tc %d, H %d, W %d)", tc, H, W);
  DC_REQUIRE_FRAMES("dc_series_bin_time", tc);
  DC_REQUIRE((long)H * W <= (1L << 30), DC_EUNSUP, "dc_series_bin_time: image %d x %d: H * W is limited to 2^30", H, W);
  if (tc == 0) return DC_OK;
  const long seen = (long)phase + tc, n_out = seen / b;
  const int rem = (int)(seen % b);
  const bool uses_carry = phase > 0 || rem > 0;          // read by slot 0, written by the open slot: otherwise never followed
  DC_REQUIRE(frames && (n_out == 0 || out) && (!uses_carry || carry), DC_EINVAL, "dc_series_bin_time: null pointer");
  DC_REQUIRE((((uintptr_t)frames | (uintptr_t)out) & 1) == 0 && (((uintptr_t)carry) & 3) == 0, DC_EINVAL, "dc_series_bin_time: misaligned buffer");
  const uintptr_t HW = (uintptr_t)H * W, fa = (uintptr_t)frames, fb = 2 * HW * (uintptr_t)tc, oa = (uintptr_t)out, ob = 2 * HW * (uintptr_t)n_out,
                  ca = (uintptr_t)carry, cb = uses_carry ? 4 * HW : 0;
  DC_REQUIRE(ob == 0 || fa + fb <= oa || oa + ob <= fa, DC_EINVAL, "dc_series_bin_time: out overlaps frames");
  DC_REQUIRE(ob == 0 || cb == 0 || ca + cb <= oa || oa + ob <= ca, DC_EINVAL, "dc_series_bin_time: out overlaps carry");
  DC_REQUIRE(cb == 0 || fa + fb <= ca || ca + cb <= fa, DC_EINVAL, "dc_series_bin_time: carry overlaps frames");
  const int ride = (int)(phase > 0 && rem > 0 && n_out > 0);      // carry is read AND written: the open slot rides on slot 0's items
  const long n_slots = n_out + (rem > 0 && !ride);
  const bool whole = HW % kBinPix == 0;
  const int wide_in = (int)(whole && dc_aligned16(frames)), wide_out = (int)(whole && dc_aligned16(out)), wide_carry = (int)dc_aligned16(carry);
  const int bx = dc_cdiv(dc_cdiv((long)HW, kBinPix), kThreads);
  const dim3 grid((unsigned)(bx < kBinBlocksX ? bx : kBinBlocksX), (unsigned)(n_slots < 65535 ? n_slots : 65535)), block(kThreads);
  const uint32_t magic = dc_series_bin_magic(b);
  const uint16_t* f = (const uint16_t*)frames;
  if (is_unsigned)
    hipLaunchKernelGGL(series_bin_time_kernel<true>, grid, block, 0, (hipStream_t)stream, f, tc, (int)HW, b, phase, magic, carry, (uint16_t*)out,
                       (int)n_out, (int)n_slots, ride, wide_in, wide_out, wide_carry);
  else
    hipLaunchKernelGGL(series_bin_time_kernel<false>, grid, block, 0, (hipStream_t)stream, f, tc, (int)HW, b, phase, magic, carry, (uint16_t*)out,
                       (int)n_out, (int)n_slots, ride, wide_in, wide_out, wide_carry);
  DC_CHECK_LAUNCH("dc_series_bin_time");
  return DC_OK;
}

extern "C" long dc_series_standardize_ws_floats(int H, int W) {
  (void)H; (void)W;
  return 2L * 2 * kStdBlocks;            // two rows of kStdBlocks doubles
}

extern "C" int dc_image_standardize(const float* in, float* out, float* ws, int H, int W, dc_stream_t stream) {
  DC_REQUIRE(in && out && ws, DC_EINVAL, "dc_image_standardize: null pointer");
  DC_REQUIRE(H > 0 && W > 0 && (long)H * W <= (1L << 30), DC_EINVAL, "dc_image_standardize: image %d x %d out of range", H, W);
  DC_REQUIRE((((uintptr_t)ws) & 7) == 0, DC_EINVAL, "dc_image_standardize: ws must be 8-byte aligned");
  const long n = (long)H * W;
  double* w = (double*)ws;
  hipLaunchKernelGGL(image_standardize_kernel<0>, dim3(kStdBlocks), dim3(kThreads), 0, (hipStream_t)stream, in, out, w, n);
  DC_CHECK_LAUNCH("dc_image_standardize(sum)");
  hipLaunchKernelGGL(image_standardize_kernel<1>, dim3(kStdBlocks), dim3(kThreads), 0, (hipStream_t)stream, in, out, w, n);
  DC_CHECK_LAUNCH("dc_image_standardize(var)");
  hipLaunchKernelGGL(image_standardize_kernel<2>, dim3(kStdBlocks), dim3(kThreads), 0, (hipStream_t)stream, in, out, w, n);
  DC_CHECK_LAUNCH("dc_image_standardize(apply)");
  return DC_OK;
}
