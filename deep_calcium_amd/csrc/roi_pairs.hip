// ROI pixel-pair correlation on the device: for every ROI the k x k matrix of the correlation over time of each of its pixels
// with each other one -- what separates two touching cells that one mask region holds together (include/dcunet.h, "ROI
// pixel-pair correlation").
//
// One pass over the recording beside dc_roi_trace_accumulate gathers the exact integer moments a_i = sum x_i and
// g_ij = sum x_i x_j (i <= j) of every ROI; dc_roi_pair_corr forms the numerators in 128-bit integers (pair_math.h,
// footprint_math.h) and rounds once.  Nothing in this file may be contracted into a fused multiply-add or reassociated: the
// pragma below and the per-file flag in _build.py.
#pragma clang fp contract(off)
#include "common.h"
#include "pair_math.h"
#include "detrend_math.h"

namespace {

const int kThreads = 256;
const int kTile = DC_ROI_PAIR_TILE;                  // pairs along one edge of a workgroup's tile
const int kBatch = DC_ROI_PAIR_BATCH;                // frames of the two pixel strips staged in LDS at a time
const int kBlk = 4;                                  // a thread owns kBlk x kBlk pairs: (kTile / kBlk)^2 threads
const int kSide = kTile / kBlk;
static_assert(kSide * kSide == kThreads, "one thread per register block of the tile");
static_assert(kThreads >= 2 * kTile, "the pixel indices of both strips are fetched in one step");
const int kCorrRows = 16;                            // workgroups that share the rows of one ROI's square in dc_roi_pair_corr

template <bool UNS>
__device__ __forceinline__ int widen(uint16_t v) { return UNS ? (int)v : (int)(int16_t)v; }

// One workgroup per tile (r, ti, tj) of kTile x kTile pairs of ROI r's square; thread (ty, tx) owns the kBlk x kBlk pairs
// i = ti * kTile + ty * kBlk + .., j = tj * kTile + tx * kBlk + .. for the whole chunk: 16 int64 accumulators in registers, and
// every state word read, added to and written once, by this thread alone -- no atomics, no partial sums whose grouping
// depends on the grid.  The two strips of pixels (rows and columns of the tile) are gathered for kBatch frames into LDS, widened
// to int: consecutive pixels of an ROI are consecutive flat indices along an image row, so the 64 gathers of a
// wave-instruction fall into a few 128-byte lines of one frame, as in roi_pixel_accumulate_kernel.  In the compute loop a wave
// reads 4 distinct 16-byte words of the row strip (broadcast) and 16 consecutive ones of the column strip: no bank conflict.
// One product of two widened 16-bit values needs up to 33 bits, so every product is formed in 64 bits.  The tile ti == tj reads
// one strip only and also owns a for its pixels.
template <bool UNS>
__global__ __launch_bounds__(kThreads) void roi_pair_accumulate_kernel(const uint16_t* __restrict__ frames, int tc,
                                                                      const int* __restrict__ roi_off, const int* __restrict__ roi_pix,
                                                                      const int64_t* __restrict__ goff, const int* __restrict__ tiles, int R,
                                                                      int64_t* __restrict__ a, int64_t* __restrict__ g, long P, long G, long HW) {
  __shared__ int sx[2][kBatch][kTile];
  __shared__ int sq[2][kTile];
  const int tid = threadIdx.x;
  const int* tile = tiles + 3L * blockIdx.x;
  const int r = tile[0], ti = tile[1], tj = tile[2];
  // sanitised: everything below is uniform over the workgroup, so a tile that is skipped is skipped by every thread
  if (r < 0 || r >= R || ti < 0 || tj < ti) return;
  const long p0 = roi_off[r], p1 = roi_off[r + 1], go = goff[r];
  if (!dc_pair_roi_ok(p0, p1, go, P, G, DC_ROI_PAIR_MAX_AREA)) return;
  const long k = p1 - p0;
  if ((long)tj * kTile >= k) return;                 // hence ti * kTile < k as well
  const bool diag = ti == tj;
  if (tid < 2 * kTile) {
    const int which = tid / kTile, lane = tid % kTile;
    const long i = (long)(which ? tj : ti) * kTile + lane;
    int q = i < k ? roi_pix[p0 + i] : -1;
    if (q < 0 || q >= HW) q = -1;                    // never dereferenced, counts as 0
    sq[which][lane] = q;
  }
  const int ty = tid / kSide, tx = tid % kSide;
  const int (*xi)[kTile] = sx[0];
  const int (*xj)[kTile] = sx[diag ? 0 : 1];
  int64_t acc[kBlk][kBlk] = {};
  int64_t sa = 0;
  const int nload = (diag ? 1 : 2) * kBatch * kTile;
  for (int f0 = 0; f0 < tc; f0 += kBatch) {
    const int nb = tc - f0 < kBatch ? tc - f0 : kBatch;
    __syncthreads();                                 // sq is written; the readers of the previous batch are done
#pragma unroll 8
    for (int e = tid; e < nload; e += kThreads) {
      const int which = e / (kBatch * kTile), f = (e / kTile) % kBatch, lane = e % kTile;
      const int q = sq[which][lane];
      sx[which][f][lane] = (f < nb && q >= 0) ? widen<UNS>(frames[(long)(f0 + f) * HW + q]) : 0;
    }
    __syncthreads();
    for (int f = 0; f < nb; ++f) {
      int vi[kBlk], vj[kBlk];
#pragma unroll
      for (int u = 0; u < kBlk; ++u) {
        vi[u] = xi[f][ty * kBlk + u];
        vj[u] = xj[f][tx * kBlk + u];
      }
#pragma unroll
      for (int u = 0; u < kBlk; ++u)
#pragma unroll
        for (int v = 0; v < kBlk; ++v) acc[u][v] += (int64_t)vi[u] * (int64_t)vj[v];
    }
    if (diag && tid < kTile)
      for (int f = 0; f < nb; ++f) sa += xi[f][tid];
  }
#pragma unroll
  for (int u = 0; u < kBlk; ++u) {
    const long i = (long)ti * kTile + ty * kBlk + u;
#pragma unroll
    for (int v = 0; v < kBlk; ++v) {
      const long j = (long)tj * kTile + tx * kBlk + v;
      if (i < k && j < k && i <= j) g[go + i * k + j] += acc[u][v];      // the lower triangle is never touched
    }
  }
  if (diag && tid < kTile) {
    const long i = (long)ti * kTile + tid;
    if (i < k) a[p0 + i] += sa;
  }
}

// moments -> the float32 matrix: workgroup (r, y) writes rows y, y + kCorrRows, .. of ROI r's square, one lane per column
__global__ __launch_bounds__(kThreads) void roi_pair_corr_kernel(const int64_t* __restrict__ a, const int64_t* __restrict__ g,
                                                                const int* __restrict__ roi_off, const int64_t* __restrict__ goff,
                                                                long P, long G, int64_t T, float* __restrict__ corr) {
  const int r = blockIdx.x;
  const long p0 = roi_off[r], p1 = roi_off[r + 1], go = goff[r];
  if (!dc_pair_roi_ok(p0, p1, go, P, G, DC_ROI_PAIR_MAX_AREA)) return;
  const long k = p1 - p0;
  for (long i = blockIdx.y; i < k; i += gridDim.y) {
    const int64_t ai = a[p0 + i], gii = g[go + i * k + i];
    for (long j = threadIdx.x; j < k; j += kThreads) {
      const long lo = i < j ? i : j, hi = i < j ? j : i;
      corr[go + i * k + j] = dc_fp_corr(dc_pair_numerators(T, ai, a[p0 + j], gii, g[go + lo * k + hi], g[go + j * k + j]));
    }
  }
}

// ---- detrended pairs: segment-pooled centred moments (include/dcunet.h, "Detrended correlations") --------------------------------
// One workgroup per tile of the accumulate kernel's tile list, so the ROI, its square and the tile's bounds are found the same
// way; the tile's kTile x kTile entries are walked row by row, consecutive lanes on consecutive 16-byte pooled words.  Entry
// (i, j), i <= j, is owned by one thread of one workgroup: it adds mult * (len * g_ij - a_i a_j) to the pooled word and clears
// g_ij for the next segment.  a is read by every tile of the ROI, so it is cleared behind the kernel, not in it.
__global__ __launch_bounds__(kThreads) void roi_pair_fold_segment_kernel(const int64_t* __restrict__ a, int64_t* __restrict__ g,
                                                                        const int* __restrict__ roi_off, const int64_t* __restrict__ goff,
                                                                        const int* __restrict__ tiles, int R, long P, long G, int64_t len,
                                                                        int64_t mult, int64_t* __restrict__ pooled) {
  const int* tile = tiles + 3L * blockIdx.x;
  const int r = tile[0], ti = tile[1], tj = tile[2];
  if (r < 0 || r >= R || ti < 0 || tj < ti) return;
  const long p0 = roi_off[r], p1 = roi_off[r + 1], go = goff[r];
  if (!dc_pair_roi_ok(p0, p1, go, P, G, DC_ROI_PAIR_MAX_AREA)) return;
  const long k = p1 - p0;
  if ((long)tj * kTile >= k) return;
  for (int e = threadIdx.x; e < kTile * kTile; e += kThreads) {
    const long i = (long)ti * kTile + e / kTile, j = (long)tj * kTile + e % kTile;
    if (i >= k || j >= k || i > j) continue;         // the lower triangle is never touched
    const long w = go + i * k + j;
    dc_i128_store(pooled, w, dc_i128_add(dc_i128_load(pooled, w), dc_detrend_term(len, mult, g[w], a[p0 + i], a[p0 + j])));
    g[w] = 0;
  }
}

// pooled numerators -> the float32 matrix, in the form of roi_pair_corr_kernel
__global__ __launch_bounds__(kThreads) void roi_pair_corr_pooled_kernel(const int64_t* __restrict__ pooled, const int* __restrict__ roi_off,
                                                                       const int64_t* __restrict__ goff, long P, long G,
                                                                       float* __restrict__ corr) {
  const int r = blockIdx.x;
  const long p0 = roi_off[r], p1 = roi_off[r + 1], go = goff[r];
  if (!dc_pair_roi_ok(p0, p1, go, P, G, DC_ROI_PAIR_MAX_AREA)) return;
  const long k = p1 - p0;
  for (long i = blockIdx.y; i < k; i += gridDim.y) {
    DcFpNum n;
    n.cxx = dc_i128_load(pooled, go + i * k + i);
    for (long j = threadIdx.x; j < k; j += kThreads) {
      const long lo = i < j ? i : j, hi = i < j ? j : i;
      n.cxl = dc_i128_load(pooled, go + lo * k + hi);
      n.cll = dc_i128_load(pooled, go + j * k + j);
      corr[go + i * k + j] = dc_fp_corr(n);
    }
  }
}

}  // namespace

extern "C" int dc_roi_pair_fold_segment(long* a, long* g, const int* roi_off, const long* goff, const int* tiles, long ntiles, int R, int P,
                                        long G, long len, long mult, long* pooled, dc_stream_t stream) {
  DC_REQUIRE(a && g && roi_off && goff && tiles && pooled, DC_EINVAL, "dc_roi_pair_fold_segment: null pointer");
  DC_REQUIRE(ntiles >= 0 && R >= 0 && P >= 0 && G >= 0, DC_EINVAL, "dc_roi_pair_fold_segment: negative count (ntiles %ld, R %d, P %d, G %ld)",
             ntiles, R, P, G);
  DC_REQUIRE((((uintptr_t)roi_off | (uintptr_t)tiles) & 3) == 0 && (((uintptr_t)goff | (uintptr_t)a | (uintptr_t)g) & 7) == 0 &&
             dc_aligned16(pooled), DC_EINVAL, "dc_roi_pair_fold_segment: misaligned buffer (the pooled words are 16-byte elements)");
  DC_REQUIRE(len >= 1 && mult >= 1, DC_EINVAL, "dc_roi_pair_fold_segment: a segment of %ld frames with mult %ld", len, mult);
  DC_REQUIRE(dc_detrend_segment_ok(len, mult), DC_EUNSUP,
             "dc_roi_pair_fold_segment: len = %ld, mult = %ld: a segment beside others is limited to %d frames, one alone to %ld", len, mult,
             DC_DETREND_MAX_SEGMENT, (long)DC_ROI_PIXEL_MAX_FRAMES);
  DC_REQUIRE(G <= DC_ROI_PAIR_MAX_STATE, DC_EUNSUP, "dc_roi_pair_fold_segment: G = %ld words of state: limited to 2^27 = %ld", G,
             (long)DC_ROI_PAIR_MAX_STATE);
  DC_REQUIRE(G <= (long)DC_ROI_PAIR_MAX_AREA * P, DC_EUNSUP,
             "dc_roi_pair_fold_segment: G = %ld exceeds %d * P = %ld: an ROI has more than %d pixels", G, DC_ROI_PAIR_MAX_AREA,
             (long)DC_ROI_PAIR_MAX_AREA * P, DC_ROI_PAIR_MAX_AREA);
  DC_REQUIRE(ntiles < (1L << 31), DC_EUNSUP, "dc_roi_pair_fold_segment: %ld tiles: one workgroup each, limited to 2^31 - 1", ntiles);
  DC_REQUIRE(ntiles <= (long)R * dc_pair_tiles_of(DC_ROI_PAIR_MAX_AREA, DC_ROI_PAIR_TILE), DC_EUNSUP,
             "dc_roi_pair_fold_segment: %ld tiles for %d ROIs: an ROI of at most %d pixels has %ld", ntiles, R, DC_ROI_PAIR_MAX_AREA,
             (long)dc_pair_tiles_of(DC_ROI_PAIR_MAX_AREA, DC_ROI_PAIR_TILE));
  if (ntiles == 0 || R == 0 || P == 0 || G == 0) return DC_OK;
  hipLaunchKernelGGL(roi_pair_fold_segment_kernel, dim3((unsigned)ntiles), dim3(kThreads), 0, (hipStream_t)stream, (const int64_t*)a, (int64_t*)g,
                     roi_off, (const int64_t*)goff, tiles, R, (long)P, G, (int64_t)len, (int64_t)mult, (int64_t*)pooled);
  DC_CHECK_LAUNCH("dc_roi_pair_fold_segment");
  const hipError_t e = hipMemsetAsync(a, 0, 8 * (size_t)P, (hipStream_t)stream);      // behind the kernel: every tile of an ROI reads its a
  DC_REQUIRE(e == hipSuccess, DC_EHIP, "dc_roi_pair_fold_segment: hipMemsetAsync: %s", hipGetErrorString(e));
  return DC_OK;
}

extern "C" int dc_roi_pair_corr_pooled(const long* pooled, const int* roi_off, const long* goff, int R, int P, long G, float* corr,
                                       dc_stream_t stream) {
  DC_REQUIRE(pooled && roi_off && goff && corr, DC_EINVAL, "dc_roi_pair_corr_pooled: null pointer");
  DC_REQUIRE(R >= 0 && P >= 0 && G >= 0, DC_EINVAL, "dc_roi_pair_corr_pooled: negative count (R %d, P %d, G %ld)", R, P, G);
  DC_REQUIRE(dc_aligned16(pooled) && (((uintptr_t)goff) & 7) == 0 && (((uintptr_t)roi_off | (uintptr_t)corr) & 3) == 0, DC_EINVAL,
             "dc_roi_pair_corr_pooled: misaligned buffer (the pooled words are 16-byte elements)");
  DC_REQUIRE(G <= DC_ROI_PAIR_MAX_STATE, DC_EUNSUP, "dc_roi_pair_corr_pooled: G = %ld words of state: limited to 2^27 = %ld", G,
             (long)DC_ROI_PAIR_MAX_STATE);
  DC_REQUIRE(G <= (long)DC_ROI_PAIR_MAX_AREA * P, DC_EUNSUP,
             "dc_roi_pair_corr_pooled: G = %ld exceeds %d * P = %ld: an ROI has more than %d pixels", G, DC_ROI_PAIR_MAX_AREA,
             (long)DC_ROI_PAIR_MAX_AREA * P, DC_ROI_PAIR_MAX_AREA);
  if (R == 0 || P == 0 || G == 0) return DC_OK;
  hipLaunchKernelGGL(roi_pair_corr_pooled_kernel, dim3((unsigned)R, kCorrRows), dim3(kThreads), 0, (hipStream_t)stream, (const int64_t*)pooled,
                     roi_off, (const int64_t*)goff, (long)P, G, corr);
  DC_CHECK_LAUNCH("dc_roi_pair_corr_pooled");
  return DC_OK;
}

extern "C" int dc_roi_pair_accumulate(const void* frames, int is_unsigned, int tc, const int* roi_off, const int* roi_pix, const long* goff,
                                      const int* tiles, long ntiles, int R, long* a, long* g, int P, long G, int H, int W,
                                      dc_stream_t stream) {
  DC_REQUIRE(frames && roi_off && roi_pix && goff && tiles && a && g, DC_EINVAL, "dc_roi_pair_accumulate: null pointer");
  DC_REQUIRE(tc >= 0 && ntiles >= 0 && R >= 0 && P >= 0 && G >= 0, DC_EINVAL,
             "dc_roi_pair_accumulate: negative count (tc %d, ntiles %ld, R %d, P %d, G %ld)", tc, ntiles, R, P, G);
  DC_REQUIRE_FRAMES("dc_roi_pair_accumulate", tc);
  DC_REQUIRE(H > 0 && W > 0 && (long)H * W <= (1L << 30), DC_EINVAL, "dc_roi_pair_accumulate: image %d x %d out of range", H, W);
  DC_REQUIRE((((uintptr_t)frames) & 1) == 0 && (((uintptr_t)roi_off | (uintptr_t)roi_pix | (uintptr_t)tiles) & 3) == 0 &&
             (((uintptr_t)goff | (uintptr_t)a | (uintptr_t)g) & 7) == 0, DC_EINVAL, "dc_roi_pair_accumulate: misaligned buffer");
  const long HW = (long)H * W;
  DC_REQUIRE(tc <= DC_ROI_TRACE_MAX_VOLUME / HW, DC_EUNSUP, "dc_roi_pair_accumulate: %d frames of %d x %d: T * H * W is limited to 2^46 = %ld",
             tc, H, W, (long)DC_ROI_TRACE_MAX_VOLUME);
  DC_REQUIRE(G <= DC_ROI_PAIR_MAX_STATE, DC_EUNSUP, "dc_roi_pair_accumulate: G = %ld words of state: limited to 2^27 = %ld", G,
             (long)DC_ROI_PAIR_MAX_STATE);
  DC_REQUIRE(G <= (long)DC_ROI_PAIR_MAX_AREA * P, DC_EUNSUP,
             "dc_roi_pair_accumulate: G = %ld exceeds %d * P = %ld: an ROI has more than %d pixels", G, DC_ROI_PAIR_MAX_AREA,
             (long)DC_ROI_PAIR_MAX_AREA * P, DC_ROI_PAIR_MAX_AREA);
  DC_REQUIRE(ntiles < (1L << 31), DC_EUNSUP, "dc_roi_pair_accumulate: %ld tiles: one workgroup each, limited to 2^31 - 1", ntiles);
  DC_REQUIRE(ntiles <= (long)R * dc_pair_tiles_of(DC_ROI_PAIR_MAX_AREA, DC_ROI_PAIR_TILE), DC_EUNSUP,
             "dc_roi_pair_accumulate: %ld tiles for %d ROIs: an ROI of at most %d pixels has %ld", ntiles, R, DC_ROI_PAIR_MAX_AREA,
             (long)dc_pair_tiles_of(DC_ROI_PAIR_MAX_AREA, DC_ROI_PAIR_TILE));
  if (ntiles == 0 || R == 0 || P == 0 || G == 0 || tc == 0) return DC_OK;
  const dim3 grid((unsigned)ntiles), block(kThreads);
  const uint16_t* f = (const uint16_t*)frames;
  if (is_unsigned)
    hipLaunchKernelGGL((roi_pair_accumulate_kernel<true>), grid, block, 0, (hipStream_t)stream, f, tc, roi_off, roi_pix, (const int64_t*)goff,
                       tiles, R, (int64_t*)a, (int64_t*)g, (long)P, G, HW);
  else
    hipLaunchKernelGGL((roi_pair_accumulate_kernel<false>), grid, block, 0, (hipStream_t)stream, f, tc, roi_off, roi_pix, (const int64_t*)goff,
                       tiles, R, (int64_t*)a, (int64_t*)g, (long)P, G, HW);
  DC_CHECK_LAUNCH("dc_roi_pair_accumulate");
  return DC_OK;
}

extern "C" int dc_roi_pair_corr(const long* a, const long* g, const int* roi_off, const long* goff, int R, int P, long G, long T, float* corr,
                                dc_stream_t stream) {
  DC_REQUIRE(a && g && roi_off && goff && corr, DC_EINVAL, "dc_roi_pair_corr: null pointer");
  DC_REQUIRE(R >= 0 && P >= 0 && G >= 0 && T >= 0, DC_EINVAL, "dc_roi_pair_corr: negative count (R %d, P %d, G %ld, T %ld)", R, P, G, T);
  DC_REQUIRE((((uintptr_t)a | (uintptr_t)g | (uintptr_t)goff) & 7) == 0 && (((uintptr_t)roi_off | (uintptr_t)corr) & 3) == 0, DC_EINVAL,
             "dc_roi_pair_corr: misaligned buffer");
  DC_REQUIRE(T <= DC_ROI_PIXEL_MAX_FRAMES, DC_EUNSUP, "dc_roi_pair_corr: T = %ld: T is limited to 2^31 - 1 = %ld", T,
             (long)DC_ROI_PIXEL_MAX_FRAMES);
  DC_REQUIRE(G <= DC_ROI_PAIR_MAX_STATE, DC_EUNSUP, "dc_roi_pair_corr: G = %ld words of state: limited to 2^27 = %ld", G,
             (long)DC_ROI_PAIR_MAX_STATE);
  DC_REQUIRE(G <= (long)DC_ROI_PAIR_MAX_AREA * P, DC_EUNSUP, "dc_roi_pair_corr: G = %ld exceeds %d * P = %ld: an ROI has more than %d pixels",
             G, DC_ROI_PAIR_MAX_AREA, (long)DC_ROI_PAIR_MAX_AREA * P, DC_ROI_PAIR_MAX_AREA);
  if (R == 0 || P == 0 || G == 0) return DC_OK;
  hipLaunchKernelGGL(roi_pair_corr_kernel, dim3((unsigned)R, kCorrRows), dim3(kThreads), 0, (hipStream_t)stream, (const int64_t*)a,
                     (const int64_t*)g, roi_off, (const int64_t*)goff, (long)P, G, (int64_t)T, corr);
  DC_CHECK_LAUNCH("dc_roi_pair_corr");
  return DC_OK;
}
