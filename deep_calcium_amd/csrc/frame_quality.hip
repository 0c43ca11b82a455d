// Per-frame quality scores on the device: for every frame of a chunk the exact integer sums over a rectangle -- sum x, sum x^2 and
// sum x * template --, the float32 mean and correlation with the template formed from them, and the gather that leaves frames
// out (include/dcunet.h, "Frame quality").  An artefact frame (a stimulation flash, a gated PMT, a z-jump) moves all pixels
// together: its mean leaves the recording's, or its correlation with the template drops; the rule is applied on the host.
//
// The sums are integers end to end, so who sums what changes no bit.  A product of two 16-bit values needs 33 bits: it is formed
// in 64 at once, and every accumulator is an int64 from the first pixel (frame_math.h derives the range).  Nothing in
// this file may be contracted into a fused multiply-add or reassociated: the pragma below and the per-file flag in _build.py.
#pragma clang fp contract(off)
#include "common.h"
#include "frame_math.h"

namespace {

const int kThreads = 256;
const int kWave = 64;
const int kWaves = kThreads / kWave;
const int kSlabRows = 32;             // rows of the rectangle one workgroup reduces per step: 64 frames of 512 rows are 1024 workgroups
const int kMaxSlabs = 1024;           // grid.x: more slabs than this are walked by a stride
const int kMaxFrames = 1024;          // grid.y: more frames than this are walked by a stride
const int kGatherBlocks = 1024;       // grid.x of the gather

template <bool UNS>
__device__ __forceinline__ int widen(uint16_t v) { return UNS ? (int)v : (int)(int16_t)v; }

__device__ __forceinline__ int64_t shfl_xor_i64(int64_t v, int o) { return (int64_t)__shfl_xor((long long)v, o); }

// the sum over the 64 lanes of a wave, in every lane (integer addition: the order does not matter)
__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) v += shfl_xor_i64(v, o);
  return v;
}

struct Acc { int64_t a, b, c; };

template <bool UNS, bool TMPL>
__device__ __forceinline__ void add_pixel(Acc& s, uint16_t xv, uint16_t tv) {
  const int64_t x = widen<UNS>(xv);
  s.a += x;
  s.b += x * x;                                        // 64-bit operands: 65535^2 does not fit an int32
  if (TMPL) s.c += x * (int64_t)widen<UNS>(tv);
}

// 8 pixels held in one 16-byte word, lowest address first
__device__ __forceinline__ uint16_t half_of(const uint4& v, int j) {
  const unsigned w = j < 2 ? v.x : (j < 4 ? v.y : (j < 6 ? v.z : v.w));
  return (uint16_t)((j & 1) ? (w >> 16) : (w & 0xffffu));
}

// moments[f] += the three sums of frame f over rows [y0, y1), columns [x0, x1).  grid = (slabs of kSlabRows rows, frames), both
// capped and strided.  A wave takes a row of its slab at a time; the row starts at an arbitrary x0, so the lanes read it as a
// scalar prologue up to the next 16-byte boundary of the FRAME's row, whole 16-byte words of 8 pixels, and a scalar epilogue --
// lane 0 takes the prologue, lane 1 the epilogue, every lane a stride of the words.  The template's row is read by 16-byte words
// too where it shares the frame row's alignment (always, for aligned bases and H * W % 8 == 0), and by 16-bit loads otherwise.
// The wave adds its sums by 64-bit shuffles, the workgroup's four waves meet in LDS, and three 64-bit atomics per workgroup and
// frame go to memory, into a row the same call zeroed.
template <bool UNS, bool TMPL>
__global__ __launch_bounds__(kThreads) void frame_moments_kernel(const uint16_t* __restrict__ frames, int tc, const uint16_t* __restrict__ tmpl,
                                                                int H, int W, int y0, int y1, int x0, int x1,
                                                                unsigned long long* __restrict__ moments, int slabs) {
  __shared__ int64_t red[kWaves][3];
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const int w = x1 - x0;
  for (int f = blockIdx.y; f < tc; f += gridDim.y) {
    const uint16_t* __restrict__ fr = frames + (long)f * H * W;
    Acc s = {0, 0, 0};
    for (int slab = blockIdx.x; slab < slabs; slab += gridDim.x) {
      const int r0 = y0 + slab * kSlabRows, r1 = r0 + kSlabRows < y1 ? r0 + kSlabRows : y1;
      for (int y = r0 + wave; y < r1; y += kWaves) {
        const uint16_t* __restrict__ xr = fr + (long)y * W + x0;
        const uint16_t* __restrict__ tr = TMPL ? tmpl + (long)y * W + x0 : nullptr;
        int lead = (int)((8 - (((uintptr_t)xr >> 1) & 7)) & 7);          // pixels in front of the first 16-byte boundary
        lead = lead < w ? lead : w;
        const int nvec = (w - lead) / 8, tail0 = lead + 8 * nvec;
        const bool twide = TMPL && ((((uintptr_t)tr - (uintptr_t)xr) & 15) == 0);
        if (lane == 0)
          for (int i = 0; i < lead; ++i) add_pixel<UNS, TMPL>(s, xr[i], TMPL ? tr[i] : (uint16_t)0);
        if (lane == 1)
          for (int i = tail0; i < w; ++i) add_pixel<UNS, TMPL>(s, xr[i], TMPL ? tr[i] : (uint16_t)0);
        for (int v = lane; v < nvec; v += kWave) {
          const int at = lead + 8 * v;
          const uint4 xv = *reinterpret_cast<const uint4*>(xr + at);
          if (!TMPL) {
#pragma unroll
            for (int j = 0; j < 8; ++j) add_pixel<UNS, false>(s, half_of(xv, j), 0);
          } else if (twide) {
            const uint4 tv = *reinterpret_cast<const uint4*>(tr + at);
#pragma unroll
            for (int j = 0; j < 8; ++j) add_pixel<UNS, true>(s, half_of(xv, j), half_of(tv, j));
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) add_pixel<UNS, true>(s, half_of(xv, j), tr[at + j]);
          }
        }
      }
    }
    s.a = wave_sum(s.a);
    s.b = wave_sum(s.b);
    if (TMPL) s.c = wave_sum(s.c);
    __syncthreads();                                   // the readers of the previous frame's totals are done
    if (lane == 0) { red[wave][0] = s.a; red[wave][1] = s.b; red[wave][2] = TMPL ? s.c : 0; }
    __syncthreads();
    if (threadIdx.x < (TMPL ? 3 : 2)) {
      int64_t t = 0;
      for (int k = 0; k < kWaves; ++k) t += red[k][threadIdx.x];
      if (t) atomicAdd(moments + 3 * (long)f + threadIdx.x, (unsigned long long)t);      // two's complement: the wrap is the sum
    }
  }
}

// moments -> float32, one thread per frame
__global__ __launch_bounds__(kThreads) void frame_quality_kernel(const int64_t* __restrict__ moments, int tc, int64_t n, int64_t ta, int64_t tb,
                                                                float* __restrict__ mean, float* __restrict__ corr) {
  for (long f = (long)blockIdx.x * kThreads + threadIdx.x; f < tc; f += (long)gridDim.x * kThreads) {
    const int64_t a = moments[3 * f], b = moments[3 * f + 1], c = moments[3 * f + 2];
    mean[f] = dc_frame_mean(a, n);
    if (corr) corr[f] = dc_fp_corr(dc_frame_numerators(n, a, b, c, ta, tb));
  }
}

// out[i] = frames[idx[i]], all zeros where idx[i] names no frame of the chunk (the index is never followed then).  grid =
// (pieces of a frame, output frames), both capped and strided.  16-byte words where the source frame and the output frame
// are both 16-byte aligned, 16-bit moves otherwise and for the last H * W % 8 pixels.
__global__ __launch_bounds__(kThreads) void frame_gather_kernel(const uint16_t* __restrict__ frames, int tc, const int* __restrict__ idx, int k,
                                                               long HW, uint16_t* __restrict__ out) {
  const long tid = (long)blockIdx.x * kThreads + threadIdx.x, step = (long)gridDim.x * kThreads;
  for (int i = blockIdx.y; i < k; i += gridDim.y) {
    const int t = idx[i];
    const bool live = t >= 0 && t < tc;
    const uint16_t* __restrict__ src = frames + (live ? (long)t * HW : 0L);
    uint16_t* __restrict__ dst = out + (long)i * HW;
    const bool wide = ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0;
    const long nvec = wide ? HW / 8 : 0;
    for (long v = tid; v < nvec; v += step)
      reinterpret_cast<uint4*>(dst)[v] = live ? reinterpret_cast<const uint4*>(src)[v] : make_uint4(0u, 0u, 0u, 0u);
    for (long p = 8 * nvec + tid; p < HW; p += step) dst[p] = live ? src[p] : (uint16_t)0;
  }
}

template <bool UNS, bool TMPL>
void launch_moments(const void* frames, int tc, const void* tmpl, int H, int W, int y0, int y1, int x0, int x1, long* moments, hipStream_t stream) {
  const int slabs = dc_cdiv(y1 - y0, kSlabRows);
  const dim3 grid((unsigned)(slabs < kMaxSlabs ? slabs : kMaxSlabs), (unsigned)(tc < kMaxFrames ? tc : kMaxFrames)), block(kThreads);
  hipLaunchKernelGGL((frame_moments_kernel<UNS, TMPL>), grid, block, 0, stream, (const uint16_t*)frames, tc, (const uint16_t*)tmpl, H, W, y0, y1,
                     x0, x1, (unsigned long long*)moments, slabs);
}

}  // namespace

extern "C" int dc_frame_moments(const void* frames, int is_unsigned, int tc, const void* tmpl, int H, int W, int y0, int y1, int x0, int x1,
                                long* moments, dc_stream_t stream) {
  DC_REQUIRE(frames && moments, DC_EINVAL, "dc_frame_moments: null pointer");
  DC_REQUIRE(tc >= 0 && H > 0 && W > 0, DC_EINVAL, "dc_frame_moments: negative or zero size (tc %d, H %d, W %d)", tc, H, W);
  DC_REQUIRE_FRAMES("dc_frame_moments", tc);
  DC_REQUIRE((long)H * W <= (1L << 30), DC_EUNSUP, "dc_frame_moments: image %d x %d: H * W is limited to 2^30", H, W);
  const int64_t n = dc_frame_rect_pixels(H, W, y0, y1, x0, x1);
  DC_REQUIRE(n > 0, DC_EINVAL, "dc_frame_moments: the rectangle [%d, %d) x [%d, %d) is empty or leaves the %d x %d frame", y0, y1, x0, x1, H, W);
  DC_REQUIRE(n <= DC_FRAME_MAX_PIXELS, DC_EUNSUP, "dc_frame_moments: a rectangle of %ld pixels: limited to 2^28 = %ld", (long)n,
             (long)DC_FRAME_MAX_PIXELS);
  DC_REQUIRE(((((uintptr_t)frames) | ((uintptr_t)tmpl)) & 1) == 0 && (((uintptr_t)moments) & 7) == 0, DC_EINVAL,
             "dc_frame_moments: misaligned buffer");
  if (tc == 0) return DC_OK;
  // the totals arrive by atomics: the rows are zeroed first, on the same stream
  const hipError_t e = hipMemsetAsync(moments, 0, 24 * (size_t)tc, (hipStream_t)stream);
  DC_REQUIRE(e == hipSuccess, DC_EHIP, "dc_frame_moments: hipMemsetAsync: %s", hipGetErrorString(e));
  if (tmpl) {
    if (is_unsigned) launch_moments<true, true>(frames, tc, tmpl, H, W, y0, y1, x0, x1, moments, (hipStream_t)stream);
    else launch_moments<false, true>(frames, tc, tmpl, H, W, y0, y1, x0, x1, moments, (hipStream_t)stream);
  } else {
    if (is_unsigned) launch_moments<true, false>(frames, tc, tmpl, H, W, y0, y1, x0, x1, moments, (hipStream_t)stream);
    else launch_moments<false, false>(frames, tc, tmpl, H, W, y0, y1, x0, x1, moments, (hipStream_t)stream);
  }
  DC_CHECK_LAUNCH("dc_frame_moments");
  return DC_OK;
}

extern "C" int dc_frame_quality(const long* moments, int tc, long n, long ta, long tb, float* mean, float* corr, dc_stream_t stream) {
  DC_REQUIRE(moments && mean, DC_EINVAL, "dc_frame_quality: null pointer");
  DC_REQUIRE(tc >= 0, DC_EINVAL, "dc_frame_quality: negative count (tc %d)", tc);
  DC_REQUIRE_FRAMES("dc_frame_quality", tc);
  DC_REQUIRE(n >= 1, DC_EINVAL, "dc_frame_quality: n = %ld pixels", n);
  DC_REQUIRE(n <= DC_FRAME_MAX_PIXELS, DC_EUNSUP, "dc_frame_quality: n = %ld pixels: limited to 2^28 = %ld", n, (long)DC_FRAME_MAX_PIXELS);
  DC_REQUIRE((((uintptr_t)moments) & 7) == 0 && ((((uintptr_t)mean) | ((uintptr_t)corr)) & 3) == 0, DC_EINVAL,
             "dc_frame_quality: misaligned buffer");
  if (tc == 0) return DC_OK;
  const int blocks = dc_cdiv(tc, kThreads);
  hipLaunchKernelGGL(frame_quality_kernel, dim3((unsigned)(blocks < kMaxFrames ? blocks : kMaxFrames)), dim3(kThreads), 0, (hipStream_t)stream,
                     (const int64_t*)moments, tc, (int64_t)n, (int64_t)ta, (int64_t)tb, mean, corr);
  DC_CHECK_LAUNCH("dc_frame_quality");
  return DC_OK;
}

extern "C" int dc_frame_gather(const void* frames, int tc, const int* idx, int k, int H, int W, void* out, dc_stream_t stream) {
  DC_REQUIRE(tc >= 0 && k >= 0 && H > 0 && W > 0, DC_EINVAL, "dc_frame_gather: negative or zero size (tc %d, k %d, H %d, W %d)", tc, k, H, W);
  DC_REQUIRE_FRAMES("dc_frame_gather", tc);
  DC_REQUIRE((long)H * W <= (1L << 30), DC_EUNSUP, "dc_frame_gather: image %d x %d: H * W is limited to 2^30", H, W);
  if (k == 0) return DC_OK;
  DC_REQUIRE(frames && idx && out, DC_EINVAL, "dc_frame_gather: null pointer");
  DC_REQUIRE(((((uintptr_t)frames) | ((uintptr_t)out)) & 1) == 0 && (((uintptr_t)idx) & 3) == 0, DC_EINVAL, "dc_frame_gather: misaligned buffer");
  const long HW = (long)H * W;
  const uintptr_t f0 = (uintptr_t)frames, f1 = f0 + 2 * (uintptr_t)HW * (uintptr_t)tc, o0 = (uintptr_t)out, o1 = o0 + 2 * (uintptr_t)HW * (uintptr_t)k;
  DC_REQUIRE(o1 <= f0 || f1 <= o0, DC_EINVAL, "dc_frame_gather: out overlaps frames");
  const int bx = dc_cdiv(dc_cdiv(HW, 8), kThreads);
  const dim3 grid((unsigned)(bx < kGatherBlocks ? bx : kGatherBlocks), (unsigned)(k < kMaxFrames ? k : kMaxFrames)), block(kThreads);
  hipLaunchKernelGGL(frame_gather_kernel, grid, block, 0, (hipStream_t)stream, (const uint16_t*)frames, tc, idx, k, HW, (uint16_t*)out);
  DC_CHECK_LAUNCH("dc_frame_gather");
  return DC_OK;
}
