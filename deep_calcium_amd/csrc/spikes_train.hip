// UNet1D training (deepcalcium/models/spikes/unet_1d_segmentation.py: unet1d :49-148 as fit :217-380 trains it), gfx950:
// the 1-D hot path of a train step that spikes.hip (inference) and elementwise.hip (BatchNorm / ReLU / Dropout / Adam on
// [pixels][C] tensors, pixels = N * T) do not already cover.
//   dc_conv1d_stats              per-channel (sum, sumsq) of the pre-BatchNorm output, double partials
//   dc_conv1d_k5_wgrad           dw of Conv1D(nbf, 5, 'same'): fp32 matrix cores, contraction over N * T split over workgroups
//   dc_conv1d_k5_c1_wgrad        the same for the 1-channel first layer (vector kernel)
//   dc_maxpool1d_2_bwd           MaxPooling1D(2) backward (argmax recomputed, first maximum wins) + the skip gradient
//   dc_upsample1d_2x_drop_fwd/_bwd   UpSampling1D + Dropout (:114-115)
//   dc_spike_head_train_fwd/_bwd     the head (:139-145) with the weighted loss and the metric sums (utils/spikes.py:11-57)
// The data gradient of a conv_layer is dc_conv1d_k5_fwd on dz with the kernel packed flipped and transposed (dcunet.h).
// Conventions of spikes.hip: channels-last fp32, nothing is read across a trace boundary, fp32 (or double) accumulation in a
// FIXED order and no atomics -- a repeated call gives the same bits.
#include "wgrad_common.h"

static int st_blocks(long total, int cap) {
  const long b = (total + 255) / 256;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// ---------------------------------------------------------------------------------------------------------------------
// BatchNorm statistics of z [pixels][C] (sample stride z_ld): partial[block][C][2] = (sum z, sum z^2) in DOUBLE, the layout
// dc_bn_stats_finalize reads with groups == 1.  256 threads = PPB sample lanes x C/4 channel quads (threads past PPB * C4
// idle); a thread adds its samples in ascending order, the sample lanes of a quad are added in lane order by lane 0.
#define STATS_MAX_BLOCKS 1024
#define STATS_SAMPLES_PER_LANE 16

__global__ __launch_bounds__(256) void conv1d_stats_kernel(const float* __restrict__ z, long z_ld, double* __restrict__ partial,
                                                           long pixels, int C) {
  __shared__ double sm[256][8];
  const int C4 = C >> 2, PPB = 256 / C4;
  const int tid = threadIdx.x, q = tid % C4, pl = tid / C4;
  double s1[4] = {0., 0., 0., 0.}, s2[4] = {0., 0., 0., 0.};
  if (pl < PPB) {
    for (long pix = (long)blockIdx.x * PPB + pl; pix < pixels; pix += (long)gridDim.x * PPB) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(z + pix * z_ld + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double d = (double)v[e];
        s1[e] += d;
        s2[e] += d * d;
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) { sm[tid][e] = s1[e]; sm[tid][4 + e] = s2[e]; }
  __syncthreads();
  if (pl == 0) {
    for (int k = 1; k < PPB; ++k)
#pragma unroll
      for (int e = 0; e < 4; ++e) { s1[e] += sm[k * C4 + q][e]; s2[e] += sm[k * C4 + q][4 + e]; }
    double* dst = partial + ((long)blockIdx.x * C + 4 * q) * 2;
#pragma unroll
    for (int e = 0; e < 4; ++e) { dst[2 * e] = s1[e]; dst[2 * e + 1] = s2[e]; }
  }
}

static int stats_blocks(long pixels, int C) {
  const int PPB = 256 / (C / 4);
  const long b = (pixels + (long)PPB * STATS_SAMPLES_PER_LANE - 1) / ((long)PPB * STATS_SAMPLES_PER_LANE);
  return (int)(b < 1 ? 1 : (b > STATS_MAX_BLOCKS ? STATS_MAX_BLOCKS : b));
}

extern "C" int dc_conv1d_stats_blocks(long pixels, int C) {
  if (pixels < 1 || C < 4 || C % 4 || C > 1024) return 0;
  return stats_blocks(pixels, C);
}

extern "C" int dc_conv1d_stats(const float* z, long z_ld, double* partial, long pixels, int C, dc_stream_t stream) {
  DC_REQUIRE(z && partial, DC_EINVAL, "dc_conv1d_stats: null pointer");
  DC_REQUIRE(dc_aligned16(z) && dc_aligned16(partial), DC_EINVAL, "dc_conv1d_stats: pointers must be 16-byte aligned");
  DC_REQUIRE(pixels >= 1, DC_EINVAL, "dc_conv1d_stats: pixels=%ld must be >= 1", pixels);
  DC_REQUIRE(C >= 4 && C % 4 == 0 && C <= 1024, DC_EINVAL, "dc_conv1d_stats: C=%d must be a multiple of 4 in 4..1024", C);
  DC_REQUIRE(z_ld >= C && z_ld % 4 == 0, DC_EINVAL, "dc_conv1d_stats: z_ld=%ld must be a multiple of 4 and >= C=%d", z_ld, C);
  hipLaunchKernelGGL(conv1d_stats_kernel, dim3(stats_blocks(pixels, C)), dim3(256), 0, (hipStream_t)stream, z, z_ld, partial,
                     pixels, C);
  DC_CHECK_LAUNCH("dc_conv1d_stats");
  return DC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// dw[tap][ci][co] = sum over (n, t) of x[n][t + tap - 2][ci] * dz[n][t][co]  -- the 1-D sibling of wgrad.hip.
// The contraction index is the sample, so the MFMA "k" runs over samples: one v_mfma_f32_32x32x2_f32 consumes two
// neighbouring samples (lane half h takes sample 2s + h) for 32 input channels x 32 output channels.  A tile is TS samples
// of ONE trace: the x tile (TS + 4 samples: a 2-sample halo either side, ZERO outside [0, T) of that trace) and the dz tile
// sit in LDS in their natural [sample][channel] order, so operand reads are ds_read_b32 of 32 consecutive channels per
// half-wave; the dz operand is shared by the five taps, each tap is a shifted window of the one staged x tile.  A wave owns
// a 32 x 32 (ci, co) block for all five taps (80 accumulator registers).  The WK = 4 / (WM * WN) waves that share a block
// split the tile's samples and are added through LDS at the end (wgrad_store).  The tiles (N * ceil(T / TS) of them) are
// split over workgroups into contiguous ranges; every workgroup writes one slab and dc_reduce_partials adds the slabs in
// a fixed order: bit-reproducible, no atomics.  At 20 x 4096 the 32 x 32 layers get 512 workgroups of ~1-2 tiles each.
template <int RS, int WM, int WN>
struct Wgrad1dCfg {
  static constexpr int TAPS = 5, PAD = 2;
  static constexpr int WK = 4 / (WM * WN);
  static constexpr int TS = WK * RS;                    // samples per tile
  static constexpr int CM = 32 * WM, CN = 32 * WN;
  static constexpr int A_FLOATS = (TS + TAPS - 1) * CM, B_FLOATS = TS * CN;
  static constexpr int RED_FLOATS = (WK - 1) * WM * WN * 16 * 64;      // wgrad_store's cross-wave scratch
  static constexpr int LDS_FLOATS = A_FLOATS + B_FLOATS > RED_FLOATS ? A_FLOATS + B_FLOATS : RED_FLOATS;
  static_assert(RS % 2 == 0, "two samples per MFMA");
  static_assert(LDS_FLOATS * 4 <= 40 * 1024, "at least two workgroups per CU");
};

template <int RS, int WM, int WN>
__global__ __launch_bounds__(256, 2) void wgrad1d_kernel(WgradParams p) {
  using Cfg = Wgrad1dCfg<RS, WM, WN>;
  constexpr int TAPS = Cfg::TAPS, WK = Cfg::WK, TS = Cfg::TS, CM = Cfg::CM, CN = Cfg::CN;
  constexpr int NH = TS + TAPS - 1;

  __shared__ __attribute__((aligned(16))) float smem[Cfg::LDS_FLOATS];
  float* ldsA = smem;
  float* ldsB = smem + Cfg::A_FLOATS;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, h = lane >> 5;
  const int wm = wave % WM, wn = (wave / WM) % WN, wk = wave / (WM * WN);
  const int m0 = blockIdx.y * CM, n0 = blockIdx.z * CN;
  const int split = blockIdx.x;
  const int T = p.Wb;                                   // WgradParams: Wa == Wb == T, Ha == Hb == 1, tilesX tiles per trace

  f32x16 acc[TAPS];
#pragma unroll
  for (int t = 0; t < TAPS; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

  const int tile_beg = split * p.tilesPerSplit;
  const int tile_end = min(tile_beg + p.tilesPerSplit, p.tilesTotal);
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  for (int tile = tile_beg; tile < tile_end; ++tile) {
    const int trace = tile / p.tilesX;
    const int t0 = (tile - trace * p.tilesX) * TS;
    {   // x: samples t0 - 2 .. t0 + TS + 1 of THIS trace, zero outside [0, T) and beyond Cm
      constexpr int C4 = CM / 4, TOTAL = NH * C4;
      const f32x4* src = reinterpret_cast<const f32x4*>(p.A + (long)trace * T * p.Cm);
      for (int idx = tid; idx < TOTAL; idx += 256) {
        const int s = idx / C4, c4 = idx - s * C4;
        const int t = t0 - Cfg::PAD + s;
        const bool ok = t >= 0 && t < T && (m0 + 4 * c4) < p.Cm;
        const f32x4 v = ok ? src[((long)t * p.Cm + m0) / 4 + c4] : zero4;
        *reinterpret_cast<f32x4*>(ldsA + s * CM + 4 * c4) = v;
      }
    }
    {   // dz: samples t0 .. t0 + TS - 1, zero past the trace's end (they then contribute nothing) and beyond Cn
      constexpr int C4 = CN / 4, TOTAL = TS * C4;
      const f32x4* src = reinterpret_cast<const f32x4*>(p.B + (long)trace * T * p.Cn);
      for (int idx = tid; idx < TOTAL; idx += 256) {
        const int s = idx / C4, c4 = idx - s * C4;
        const int t = t0 + s;
        const bool ok = t < T && (n0 + 4 * c4) < p.Cn;
        const f32x4 v = ok ? src[((long)t * p.Cn + n0) / 4 + c4] : zero4;
        *reinterpret_cast<f32x4*>(ldsB + s * CN + 4 * c4) = v;
      }
    }
    __syncthreads();

    const float* bptr = ldsB + (wk * RS + h) * CN + wn * 32 + li;
    const float* aptr = ldsA + (wk * RS + h) * CM + wm * 32 + li;
#pragma unroll 4
    for (int s = 0; s < RS / 2; ++s) {
      const float b = bptr[2 * s * CN];
#pragma unroll
      for (int tap = 0; tap < TAPS; ++tap) {
        const float a = aptr[(2 * s + tap) * CM];       // staged sample index (2s + h) + tap  <=>  t + tap - 2
        acc[tap] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[tap], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  wgrad_store<TAPS, WM, WN, WK>(p, acc, reinterpret_cast<char*>(smem), split, m0, n0, wm, wn, wk, lane, 1.f);
}

struct Wgrad1dPlan {
  int tilesT, tilesTotal, tilesPerSplit, splits, gm, gn;
};

template <int RS, int WM, int WN>
static Wgrad1dPlan wgrad1d_plan(int N, int T, int Cin, int Cout) {
  using Cfg = Wgrad1dCfg<RS, WM, WN>;
  Wgrad1dPlan pl;
  pl.tilesT = dc_cdiv(T, Cfg::TS);
  pl.tilesTotal = N * pl.tilesT;
  pl.gm = dc_cdiv(Cin, Cfg::CM);
  pl.gn = dc_cdiv(Cout, Cfg::CN);
  int want = dc_cdiv(512, pl.gm * pl.gn);     // 2 workgroups per CU x 256 CUs: one resident round, fewest slabs
  if (want > pl.tilesTotal) want = pl.tilesTotal;
  if (want < 1) want = 1;
  pl.tilesPerSplit = dc_cdiv(pl.tilesTotal, want);
  pl.splits = dc_cdiv(pl.tilesTotal, pl.tilesPerSplit);
  return pl;
}

template <int RS, int WM, int WN>
static long wgrad1d_ws(int N, int T, int Cin, int Cout) {
  const Wgrad1dPlan pl = wgrad1d_plan<RS, WM, WN>(N, T, Cin, Cout);
  const long L = 5L * Cin * Cout;
  return (long)pl.splits * L + 32 * L;        // slabs + dc_reduce_partials' second-stage scratch
}

template <int RS, int WM, int WN>
static int wgrad1d_parts(int N, int T, int Cin, int Cout) {
  return wgrad1d_plan<RS, WM, WN>(N, T, Cin, Cout).splits;
}

template <int RS, int WM, int WN>
static int wgrad1d_launch(const float* x, const float* dz, float* dw, float* ws, int N, int T, int Cin, int Cout,
                          hipStream_t st) {
  const Wgrad1dPlan pl = wgrad1d_plan<RS, WM, WN>(N, T, Cin, Cout);
  WgradParams p{};
  p.A = x; p.B = dz; p.slabs = ws;
  p.N = N; p.Ha = 1; p.Wa = T; p.Cm = Cin; p.Hb = 1; p.Wb = T; p.Cn = Cout;
  p.tilesX = pl.tilesT; p.tilesY = 1; p.tilesTotal = pl.tilesTotal; p.tilesPerSplit = pl.tilesPerSplit;
  dim3 grid((unsigned)pl.splits, (unsigned)pl.gm, (unsigned)pl.gn);
  hipLaunchKernelGGL((wgrad1d_kernel<RS, WM, WN>), grid, dim3(256), 0, st, p);
  DC_CHECK_LAUNCH("dc_conv1d_k5_wgrad");
  const long L = 5L * Cin * Cout;
  return dc_reduce_partials(ws, pl.splits, L, 1.0f, dw, ws + (long)pl.splits * L, (dc_stream_t)st);
}

// the (ci, co) wave arrangement from the channel counts; 64 (WK == 1, 2) or 128 (WK == 4) samples per tile
#define WGRAD1D_DISPATCH(FN, ...)                                   \
  if (Cin > 32 && Cout > 32) return FN<64, 2, 2>(__VA_ARGS__);      \
  if (Cin > 32) return FN<32, 2, 1>(__VA_ARGS__);                   \
  if (Cout > 32) return FN<32, 1, 2>(__VA_ARGS__);                  \
  return FN<32, 1, 1>(__VA_ARGS__);

static long wgrad1d_ws_impl(int N, int T, int Cin, int Cout) { WGRAD1D_DISPATCH(wgrad1d_ws, N, T, Cin, Cout) }
static int wgrad1d_parts_impl(int N, int T, int Cin, int Cout) { WGRAD1D_DISPATCH(wgrad1d_parts, N, T, Cin, Cout) }
static int wgrad1d_impl(const float* x, const float* dz, float* dw, float* ws, int N, int T, int Cin, int Cout, hipStream_t st) {
  WGRAD1D_DISPATCH(wgrad1d_launch, x, dz, dw, ws, N, T, Cin, Cout, st)
}

static bool wgrad1d_shape_ok(int N, int T, int Cin, int Cout) {
  return N >= 1 && T >= 1 && Cin >= 4 && Cin % 4 == 0 && Cout >= 4 && Cout % 4 == 0 && (long)T * Cin < (1L << 31) &&
         (long)T * Cout < (1L << 31) && (long)N * dc_cdiv(T, 64) < (1L << 30) && 5L * Cin * Cout < (1L << 31);
}

extern "C" long dc_conv1d_k5_wgrad_ws_floats(int N, int T, int Cin, int Cout) {
  if (!wgrad1d_shape_ok(N, T, Cin, Cout)) return 0;
  return wgrad1d_ws_impl(N, T, Cin, Cout);
}
// how many workgroups the contraction over N * T is split over (= slabs in the workspace)
extern "C" int dc_conv1d_k5_wgrad_blocks(int N, int T, int Cin, int Cout) {
  if (!wgrad1d_shape_ok(N, T, Cin, Cout)) return 0;
  return wgrad1d_parts_impl(N, T, Cin, Cout);
}
extern "C" int dc_conv1d_k5_wgrad(const float* x, const float* dz, float* dw, float* ws, int N, int T, int Cin, int Cout,
                                  dc_stream_t stream) {
  DC_REQUIRE(x && dz && dw && ws, DC_EINVAL, "dc_conv1d_k5_wgrad: null pointer");
  DC_REQUIRE(dc_aligned16(x) && dc_aligned16(dz) && dc_aligned16(dw) && dc_aligned16(ws), DC_EINVAL,
             "dc_conv1d_k5_wgrad: pointers must be 16-byte aligned");
  DC_REQUIRE(N >= 1 && T >= 1, DC_EINVAL, "dc_conv1d_k5_wgrad: N=%d and T=%d must be >= 1", N, T);
  DC_REQUIRE(Cin >= 4 && Cin % 4 == 0 && Cout >= 4 && Cout % 4 == 0, DC_EINVAL,
             "dc_conv1d_k5_wgrad: Cin=%d and Cout=%d must be positive multiples of 4", Cin, Cout);
  DC_REQUIRE(wgrad1d_shape_ok(N, T, Cin, Cout), DC_EUNSUP, "dc_conv1d_k5_wgrad: shape exceeds 2^31 elements");
  return wgrad1d_impl(x, dz, dw, ws, N, T, Cin, Cout, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// First layer (Cin == 1): dw[tap][0][co] = sum over (n, t) of x[n][t + tap - 2] * dz[n][t][co]; x is the (N, T) trace matrix.
// 256 threads = PPB sample lanes x Cout/4 channel quads; a thread walks its samples s = n * T + t in ascending order with
// 20 fmaf accumulators (5 taps x 4 channels), the lanes of a quad are added in lane order, one slab per workgroup, the slabs
// by dc_reduce_partials.
#define C1W_MAX_BLOCKS 512
#define C1W_SAMPLES_PER_LANE 32

__global__ __launch_bounds__(256) void conv1d_c1_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dz,
                                                              float* __restrict__ slabs, int T, long total, int Cout) {
  __shared__ float sm[256][20];
  const int C4 = Cout >> 2, PPB = 256 / C4;
  const int tid = threadIdx.x, q = tid % C4, pl = tid / C4;
  float acc[5][4];
#pragma unroll
  for (int tap = 0; tap < 5; ++tap)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[tap][e] = 0.f;
  if (pl < PPB) {
    for (long s = (long)blockIdx.x * PPB + pl; s < total; s += (long)gridDim.x * PPB) {
      const int t = (int)(s % T);
      const float* xr = x + (s - t);        // this trace
      const f32x4 g = *reinterpret_cast<const f32x4*>(dz + s * Cout + 4 * q);
#pragma unroll
      for (int tap = 0; tap < 5; ++tap) {
        const int u = t + tap - 2;
        const float xv = (u >= 0 && u < T) ? xr[u] : 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[tap][e] = __builtin_fmaf(xv, g[e], acc[tap][e]);
      }
    }
  }
#pragma unroll
  for (int tap = 0; tap < 5; ++tap)
#pragma unroll
    for (int e = 0; e < 4; ++e) sm[tid][tap * 4 + e] = acc[tap][e];
  __syncthreads();
  if (pl == 0) {
    for (int k = 1; k < PPB; ++k)
#pragma unroll
      for (int tap = 0; tap < 5; ++tap)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[tap][e] += sm[k * C4 + q][tap * 4 + e];
    float* dst = slabs + (long)blockIdx.x * 5 * Cout + 4 * q;
#pragma unroll
    for (int tap = 0; tap < 5; ++tap)
#pragma unroll
      for (int e = 0; e < 4; ++e) dst[tap * Cout + e] = acc[tap][e];
  }
}

static int c1w_blocks(long total, int Cout) {
  const int PPB = 256 / (Cout / 4);
  const long b = (total + (long)PPB * C1W_SAMPLES_PER_LANE - 1) / ((long)PPB * C1W_SAMPLES_PER_LANE);
  return (int)(b < 1 ? 1 : (b > C1W_MAX_BLOCKS ? C1W_MAX_BLOCKS : b));
}

extern "C" long dc_conv1d_k5_c1_wgrad_ws_floats(int N, int T, int Cout) {
  if (N < 1 || T < 1 || Cout < 4 || Cout % 4 || Cout > 1024) return 0;
  const long L = 5L * Cout;
  return (long)c1w_blocks((long)N * T, Cout) * L + 32 * L;
}

extern "C" int dc_conv1d_k5_c1_wgrad(const float* x, const float* dz, float* dw, float* ws, int N, int T, int Cout,
                                     dc_stream_t stream) {
  DC_REQUIRE(x && dz && dw && ws, DC_EINVAL, "dc_conv1d_k5_c1_wgrad: null pointer");
  DC_REQUIRE(dc_aligned16(dz) && dc_aligned16(ws), DC_EINVAL, "dc_conv1d_k5_c1_wgrad: dz and ws must be 16-byte aligned");
  DC_REQUIRE(N >= 1 && T >= 1, DC_EINVAL, "dc_conv1d_k5_c1_wgrad: N=%d and T=%d must be >= 1", N, T);
  DC_REQUIRE(Cout >= 4 && Cout % 4 == 0 && Cout <= 1024, DC_EINVAL,
             "dc_conv1d_k5_c1_wgrad: Cout=%d must be a multiple of 4 in 4..1024", Cout);
  const long total = (long)N * T;
  const int blocks = c1w_blocks(total, Cout);
  const long L = 5L * Cout;
  hipLaunchKernelGGL(conv1d_c1_wgrad_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, dz, ws, T, total, Cout);
  DC_CHECK_LAUNCH("dc_conv1d_k5_c1_wgrad");
  return dc_reduce_partials(ws, blocks, L, 1.0f, dw, ws + (long)blocks * L, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// MaxPooling1D(2, strides=2) backward (:93) plus the skip connection's gradient: the pooled tensor's input is also a skip
// tensor, so its gradient is the routed dy plus the [2C, 3C) slice of the decoder conv's dx.
//   dx[n][2t + i][c] = (i == argmax ? dy[n][t][c] : 0) + skip[n][2t + i][c]
// The argmax is recomputed from the stored forward input `in` (the FIRST of two equal values wins: in[2t] >= in[2t+1] -> 0;
// post-ReLU and dropped zeros tie often).  An odd last sample was dropped by the forward: it gets its skip gradient only.
__global__ __launch_bounds__(256) void maxpool1d_2_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ in,
                                                              long in_ld, const float* __restrict__ skip, long skip_ld,
                                                              float* __restrict__ dx, long dx_ld, int T, int Tp, int C4,
                                                              long total) {
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cg = (int)(i % C4);
    const long s = i / C4;            // n * Tp + t, Tp = ceil(T / 2) sample pairs per trace
    const long n = s / Tp;
    const int t = (int)(s - n * Tp);
    const long row = n * T + 2 * t;
    const bool pair = 2 * t + 1 < T;
    f32x4 g0 = skip ? *reinterpret_cast<const f32x4*>(skip + row * skip_ld + 4 * cg) : zero4;
    if (pair) {
      f32x4 g1 = skip ? *reinterpret_cast<const f32x4*>(skip + (row + 1) * skip_ld + 4 * cg) : zero4;
      const f32x4 a = *reinterpret_cast<const f32x4*>(in + row * in_ld + 4 * cg);
      const f32x4 b = *reinterpret_cast<const f32x4*>(in + (row + 1) * in_ld + 4 * cg);
      const f32x4 d = *reinterpret_cast<const f32x4*>(dy + ((n * (T >> 1) + t) * (long)C4 + cg) * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (b[e] > a[e]) g1[e] += d[e]; else g0[e] += d[e];
      }
      *reinterpret_cast<f32x4*>(dx + (row + 1) * dx_ld + 4 * cg) = g1;
    }
    *reinterpret_cast<f32x4*>(dx + row * dx_ld + 4 * cg) = g0;
  }
}

extern "C" int dc_maxpool1d_2_bwd(const float* dy, const float* in, long in_ld, const float* skip, long skip_ld, float* dx,
                                  long dx_ld, int N, int T, int C, dc_stream_t stream) {
  DC_REQUIRE(in && dx && (dy || T == 1), DC_EINVAL, "dc_maxpool1d_2_bwd: null pointer");
  DC_REQUIRE(dc_aligned16(dy) && dc_aligned16(in) && dc_aligned16(skip) && dc_aligned16(dx), DC_EINVAL,
             "dc_maxpool1d_2_bwd: pointers must be 16-byte aligned");
  DC_REQUIRE(N >= 1 && T >= 1, DC_EINVAL, "dc_maxpool1d_2_bwd: N=%d and T=%d must be >= 1", N, T);
  DC_REQUIRE(C >= 4 && C % 4 == 0, DC_EINVAL, "dc_maxpool1d_2_bwd: C=%d must be a positive multiple of 4", C);
  DC_REQUIRE(in_ld >= C && in_ld % 4 == 0, DC_EINVAL, "dc_maxpool1d_2_bwd: in_ld=%ld must be a multiple of 4 and >= C=%d", in_ld, C);
  DC_REQUIRE(dx_ld >= C && dx_ld % 4 == 0, DC_EINVAL, "dc_maxpool1d_2_bwd: dx_ld=%ld must be a multiple of 4 and >= C=%d", dx_ld, C);
  DC_REQUIRE(!skip || (skip_ld >= C && skip_ld % 4 == 0), DC_EINVAL,
             "dc_maxpool1d_2_bwd: skip_ld=%ld must be a multiple of 4 and >= C=%d", skip_ld, C);
  const int Tp = (T + 1) / 2;
  const long total = (long)N * Tp * (C / 4);
  hipLaunchKernelGGL(maxpool1d_2_bwd_kernel, dim3(st_blocks(total, 8192)), dim3(256), 0, (hipStream_t)stream, dy, in, in_ld, skip,
                     skip_ld, dx, dx_ld, T, Tp, C / 4, total);
  DC_CHECK_LAUNCH("dc_maxpool1d_2_bwd");
  return DC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// UpSampling1D() followed by Dropout (:114-115 and the three decoder levels after it).  The dropout element index is that of
// the DENSE up-sampled tensor [N][2T][C] (elem = (n * 2T + u) * C + c), mask / seed conventions of dc_bn_relu_drop_fwd.
__device__ __forceinline__ f32x4 up1d_factor(const uint8_t* __restrict__ mask, uint64_t seed, float keep, float inv_keep, long elem) {
  f32x4 f;
  if (mask) {
    const uchar4 m = *reinterpret_cast<const uchar4*>(mask + elem);
    f[0] = m.x ? inv_keep : 0.f; f[1] = m.y ? inv_keep : 0.f; f[2] = m.z ? inv_keep : 0.f; f[3] = m.w ? inv_keep : 0.f;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) f[e] = dc_keep_factor(seed, (uint64_t)(elem + e), keep, inv_keep);
  }
  return f;
}

__global__ __launch_bounds__(256) void upsample1d_2x_drop_fwd_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                     long out_ld, const uint8_t* __restrict__ mask, float keep,
                                                                     uint64_t seed, int C4, long total) {
  const bool drop = keep < 1.f;
  const float inv_keep = drop ? 1.f / keep : 1.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cg = (int)(i % C4);
    const long s = i / C4;            // n * T + t: output samples 2s and 2s + 1
    const f32x4 v = reinterpret_cast<const f32x4*>(in)[i];
    f32x4 v0 = v, v1 = v;
    if (drop) {
      const long elem = (2 * s * C4 + cg) * 4;
      v0 *= up1d_factor(mask, seed, keep, inv_keep, elem);
      v1 *= up1d_factor(mask, seed, keep, inv_keep, elem + 4L * C4);
    }
    float* dst = out + 2 * s * out_ld + 4 * cg;
    *reinterpret_cast<f32x4*>(dst) = v0;
    *reinterpret_cast<f32x4*>(dst + out_ld) = v1;
  }
}

__global__ __launch_bounds__(256) void upsample1d_2x_drop_bwd_kernel(const float* __restrict__ dout, long dout_ld,
                                                                     const uint8_t* __restrict__ mask, float keep, uint64_t seed,
                                                                     float* __restrict__ din, int C4, long total) {
  const bool drop = keep < 1.f;
  const float inv_keep = drop ? 1.f / keep : 1.f;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cg = (int)(i % C4);
    const long s = i / C4;
    const float* src = dout + 2 * s * dout_ld + 4 * cg;
    f32x4 g0 = *reinterpret_cast<const f32x4*>(src), g1 = *reinterpret_cast<const f32x4*>(src + dout_ld);
    if (drop) {
      const long elem = (2 * s * C4 + cg) * 4;
      g0 *= up1d_factor(mask, seed, keep, inv_keep, elem);
      g1 *= up1d_factor(mask, seed, keep, inv_keep, elem + 4L * C4);
    }
    reinterpret_cast<f32x4*>(din)[i] = g0 + g1;
  }
}

static int up1d_check(const char* fn, const void* a, const void* b, const void* mask, long ld, float keep, int N, int T, int C) {
  DC_REQUIRE(a && b, DC_EINVAL, "%s: null pointer", fn);
  DC_REQUIRE(dc_aligned16(a) && dc_aligned16(b) && (((uintptr_t)mask) & 3) == 0, DC_EINVAL,
             "%s: tensors must be 16-byte aligned, the mask 4-byte aligned", fn);
  DC_REQUIRE(N >= 1 && T >= 1, DC_EINVAL, "%s: N=%d and T=%d must be >= 1", fn, N, T);
  DC_REQUIRE(C >= 4 && C % 4 == 0, DC_EINVAL, "%s: C=%d must be a positive multiple of 4", fn, C);
  DC_REQUIRE(ld >= C && ld % 4 == 0, DC_EINVAL, "%s: ld=%ld must be a multiple of 4 and >= C=%d", fn, ld, C);
  DC_REQUIRE(keep > 0.f, DC_EINVAL, "%s: keep=%g must be > 0", fn, (double)keep);
  return DC_OK;
}

extern "C" int dc_upsample1d_2x_drop_fwd(const float* in, float* out, long out_ld, const uint8_t* mask, float keep, uint64_t seed,
                                         int N, int T, int C, dc_stream_t stream) {
  if (int rc = up1d_check("dc_upsample1d_2x_drop_fwd", in, out, mask, out_ld, keep, N, T, C)) return rc;
  const long total = (long)N * T * (C / 4);
  hipLaunchKernelGGL(upsample1d_2x_drop_fwd_kernel, dim3(st_blocks(total, 8192)), dim3(256), 0, (hipStream_t)stream, in, out,
                     out_ld, mask, keep, seed, C / 4, total);
  DC_CHECK_LAUNCH("dc_upsample1d_2x_drop_fwd");
  return DC_OK;
}

extern "C" int dc_upsample1d_2x_drop_bwd(const float* dout, long dout_ld, const uint8_t* mask, float keep, uint64_t seed,
                                         float* din, int N, int T, int C, dc_stream_t stream) {
  if (int rc = up1d_check("dc_upsample1d_2x_drop_bwd", dout, din, mask, dout_ld, keep, N, T, C)) return rc;
  const long total = (long)N * T * (C / 4);
  hipLaunchKernelGGL(upsample1d_2x_drop_bwd_kernel, dim3(st_blocks(total, 8192)), dim3(256), 0, (hipStream_t)stream, dout,
                     dout_ld, mask, keep, seed, din, C / 4, total);
  DC_CHECK_LAUNCH("dc_upsample1d_2x_drop_bwd");
  return DC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The head in training.  Logits, 'SAME' window and p exactly as spike_head_kernel (spikes.hip) forms them -- the same
// expressions in the same order, so p is the same bits --, then per sample, with d = m0 - m1, p = 1 / (1 + exp(d)) and
// q = 1 - p = 1 / (1 + exp(-d)) (formed from d, not by subtraction: it keeps its digits where p rounds to 1):
//   loss  l = -(wpos * y * log(p + 1e-7) + wneg * (1 - y) * log(q + 1e-7))       utils/spikes.py:11-27
//   sums  {l, round(p) * y, round(p), clip(y - round(p), 0, 1), y}               :30-57, round half to even
// Block sums are a fixed tree over the workgroup's threads: partial[block][8] (3 spare), block = trace * tiles + tile.
#define HEADT_TT 192          // forward: output samples per workgroup (+ up to 63 of window reach = 255 logits)
#define HEADT_BTT 128         // backward: + 2 * 63 of reach = 254 logits
#define HEADT_MAX_POOL 64
#define HEADT_SUMS 8

__device__ __forceinline__ void head_logits(const float* __restrict__ row, const float* __restrict__ kh,
                                            const float* __restrict__ bh, int C, float& s0, float& s1) {
  const f32x4* r4 = reinterpret_cast<const f32x4*>(row);
  s0 = bh[0];
  s1 = bh[1];
  for (int cg = 0; cg < (C >> 2); ++cg) {
    const f32x4 v = r4[cg];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s0 = __builtin_fmaf(v[e], kh[(4 * cg + e) * 2 + 0], s0);
      s1 = __builtin_fmaf(v[e], kh[(4 * cg + e) * 2 + 1], s1);
    }
  }
}

__global__ __launch_bounds__(256) void spike_head_train_fwd_kernel(const float* __restrict__ a, const float* __restrict__ kh,
                                                                   const float* __restrict__ bh, int pool,
                                                                   const uint8_t* __restrict__ y, float wpos, float wneg,
                                                                   float* __restrict__ p, float* __restrict__ partial, int T,
                                                                   int C, int tilesT) {
  __shared__ float l0[256], l1[256];
  __shared__ float red[5][256];
  const int trace = blockIdx.x / tilesT;
  const int t0 = (blockIdx.x - trace * tilesT) * HEADT_TT;
  const int left = (pool - 1) / 2, right = pool / 2;
  const int tid = threadIdx.x;
  const int u = t0 - left + tid;
  if (tid < HEADT_TT + left + right && u >= 0 && u < T) {
    float s0, s1;
    head_logits(a + ((long)trace * T + u) * C, kh, bh, C, s0, s1);
    l0[tid] = s0;
    l1[tid] = s1;
  }
  __syncthreads();
  const int t = t0 + tid;
  float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (tid < HEADT_TT && t < T) {
    const int lo = max(0, t - left), hi = min(T - 1, t + right);
    float m0 = l0[lo - (t0 - left)], m1 = l1[lo - (t0 - left)];
    for (int w = lo + 1; w <= hi; ++w) {
      m0 = fmaxf(m0, l0[w - (t0 - left)]);
      m1 = fmaxf(m1, l1[w - (t0 - left)]);
    }
    const float d = m0 - m1;
    const float pv = 1.f / (1.f + expf(d));
    const float qv = 1.f / (1.f + expf(-d));
    p[(long)trace * T + t] = pv;
    const float yv = y[(long)trace * T + t] ? 1.f : 0.f;
    const float rp = rintf(pv);
    v[0] = -(wpos * yv * logf(pv + 1e-7f) + wneg * (1.f - yv) * logf(qv + 1e-7f));
    v[1] = rp * yv;
    v[2] = rp;
    v[3] = fminf(fmaxf(yv - rp, 0.f), 1.f);
    v[4] = yv;
  }
#pragma unroll
  for (int k = 0; k < 5; ++k) red[k][tid] = v[k];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s)
#pragma unroll
      for (int k = 0; k < 5; ++k) red[k][tid] += red[k][tid + s];
    __syncthreads();
  }
  if (tid < HEADT_SUMS) partial[(long)blockIdx.x * HEADT_SUMS + tid] = tid < 5 ? red[tid][0] : 0.f;
}

// Backward.  dp = dl/dp / (N * T); dm1 = dp * p * q; dm0 = -dm1; each dm_j[t] goes to the FIRST maximal logit of t's window,
// written as a gather so that no atomics are needed:  dl_j[s] = sum over t in [s - pool/2, s + (pool-1)/2] with
// argmax_j(t) == s of dm_j[t], in ascending t.  Then da[s][c] = dl_0[s] kh[c][0] + dl_1[s] kh[c][1], and the block's share
// of the head's own gradient: grad_partial[block][2C + 2] = (dkh[c][j] = sum_s a[s][c] dl_j[s] ..., dbh[j] = sum_s dl_j[s]),
// both in ascending s -- the flat (kernel, bias) order, so dc_reduce_partials over the blocks yields the two arrays.
// A workgroup owns HEADT_BTT samples s and needs the logits of s +- (pool - 1): the window of every t whose window holds s.
__global__ __launch_bounds__(256) void spike_head_train_bwd_kernel(const float* __restrict__ a, const float* __restrict__ kh,
                                                                   const float* __restrict__ bh, int pool,
                                                                   const uint8_t* __restrict__ y, float wpos, float wneg,
                                                                   float inv_count, float* __restrict__ da,
                                                                   float* __restrict__ grad_partial, int T, int C, int tilesT) {
  __shared__ float l0[256], l1[256];
  __shared__ float dm[256];          // dm1 of sample t = tbase + index
  __shared__ int am0[256], am1[256]; // first argmax (absolute sample) of each logit channel over t's window
  __shared__ float dl0[HEADT_BTT], dl1[HEADT_BTT];
  const int trace = blockIdx.x / tilesT;
  const int t0 = (blockIdx.x - trace * tilesT) * HEADT_BTT;
  const int left = (pool - 1) / 2, right = pool / 2;
  const int tid = threadIdx.x;
  const int ubase = t0 - (pool - 1);          // first sample whose logits are formed
  const int tbase = t0 - right;               // first t whose window can hold a sample of this tile
  {
    const int u = ubase + tid;
    if (tid < HEADT_BTT + 2 * (pool - 1) && u >= 0 && u < T) {
      float s0, s1;
      head_logits(a + ((long)trace * T + u) * C, kh, bh, C, s0, s1);
      l0[tid] = s0;
      l1[tid] = s1;
    }
  }
  __syncthreads();
  {
    const int t = tbase + tid;
    if (tid < HEADT_BTT + pool - 1 && t >= 0 && t < T) {
      const int lo = max(0, t - left), hi = min(T - 1, t + right);     // inside [ubase, ubase + BTT + 2 (pool - 1))
      float m0 = l0[lo - ubase], m1 = l1[lo - ubase];
      int i0 = lo, i1 = lo;
      for (int w = lo + 1; w <= hi; ++w) {
        const float c0 = l0[w - ubase], c1 = l1[w - ubase];
        if (c0 > m0) { m0 = c0; i0 = w; }
        if (c1 > m1) { m1 = c1; i1 = w; }
      }
      const float d = m0 - m1;
      const float pv = 1.f / (1.f + expf(d));
      const float qv = 1.f / (1.f + expf(-d));
      const bool pos = y[(long)trace * T + t] != 0;
      const float dldp = pos ? -wpos / (pv + 1e-7f) : wneg / (qv + 1e-7f);
      dm[tid] = dldp * inv_count * pv * qv;
      am0[tid] = i0;
      am1[tid] = i1;
    }
  }
  __syncthreads();
  const int s = t0 + tid;
  if (tid < HEADT_BTT) {
    float g0 = 0.f, g1 = 0.f;
    if (s < T) {
      const int lo = max(0, s - right), hi = min(T - 1, s + left);
      for (int t = lo; t <= hi; ++t) {
        const float g = dm[t - tbase];
        if (am0[t - tbase] == s) g0 -= g;
        if (am1[t - tbase] == s) g1 += g;
      }
      f32x4* dst = reinterpret_cast<f32x4*>(da + ((long)trace * T + s) * C);
      for (int cg = 0; cg < (C >> 2); ++cg) {
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          o[e] = __builtin_fmaf(g0, kh[(4 * cg + e) * 2 + 0], g1 * kh[(4 * cg + e) * 2 + 1]);
        dst[cg] = o;
      }
    }
    dl0[tid] = g0;
    dl1[tid] = g1;
  }
  __syncthreads();
  const int ns = min(HEADT_BTT, T - t0);
  float* gp = grad_partial + (long)blockIdx.x * (2 * C + 2);
  for (int idx = tid; idx < 2 * C + 2; idx += 256) {
    const float* dl = (idx & 1) ? dl1 : dl0;
    float acc = 0.f;
    if (idx < 2 * C) {
      const float* col = a + ((long)trace * T + t0) * C + (idx >> 1);
      for (int k = 0; k < ns; ++k) acc = __builtin_fmaf(col[(long)k * C], dl[k], acc);
    } else {
      for (int k = 0; k < ns; ++k) acc += dl[k];
    }
    gp[idx] = acc;
  }
}

static int head_train_check(const char* fn, const void* a, const void* kh, const void* bh, const void* y, const void* o1,
                            const void* o2, int pool, int N, int T, int C) {
  DC_REQUIRE(a && kh && bh && y && o1 && o2, DC_EINVAL, "%s: null pointer", fn);
  DC_REQUIRE(dc_aligned16(a), DC_EINVAL, "%s: a must be 16-byte aligned", fn);
  DC_REQUIRE(N >= 1 && T >= 1, DC_EINVAL, "%s: N=%d and T=%d must be >= 1", fn, N, T);
  DC_REQUIRE(C >= 4 && C % 4 == 0, DC_EINVAL, "%s: C=%d must be a positive multiple of 4", fn, C);
  DC_REQUIRE(pool >= 1 && pool <= HEADT_MAX_POOL, DC_EINVAL, "%s: pool=%d must be in 1..%d", fn, pool, HEADT_MAX_POOL);
  DC_REQUIRE((long)N * dc_cdiv(T, HEADT_BTT) < (1L << 31), DC_EUNSUP, "%s: too many workgroups", fn);
  return DC_OK;
}

extern "C" int dc_spike_head_train_fwd_blocks(int N, int T) {
  return (N < 1 || T < 1 || (long)N * dc_cdiv(T, HEADT_TT) >= (1L << 31)) ? 0 : N * dc_cdiv(T, HEADT_TT);
}
extern "C" int dc_spike_head_train_bwd_blocks(int N, int T) {
  return (N < 1 || T < 1 || (long)N * dc_cdiv(T, HEADT_BTT) >= (1L << 31)) ? 0 : N * dc_cdiv(T, HEADT_BTT);
}

extern "C" int dc_spike_head_train_fwd(const float* a, const float* kh, const float* bh, int pool, const uint8_t* y, float wpos,
                                       float wneg, float* p, float* partial, int N, int T, int C, dc_stream_t stream) {
  if (int rc = head_train_check("dc_spike_head_train_fwd", a, kh, bh, y, p, partial, pool, N, T, C)) return rc;
  const int tilesT = dc_cdiv(T, HEADT_TT);
  hipLaunchKernelGGL(spike_head_train_fwd_kernel, dim3((unsigned)(N * tilesT)), dim3(256), 0, (hipStream_t)stream, a, kh, bh, pool,
                     y, wpos, wneg, p, partial, T, C, tilesT);
  DC_CHECK_LAUNCH("dc_spike_head_train_fwd");
  return DC_OK;
}

extern "C" int dc_spike_head_train_bwd(const float* a, const float* kh, const float* bh, int pool, const uint8_t* y, float wpos,
                                       float wneg, float* da, float* grad_partial, int N, int T, int C, dc_stream_t stream) {
  if (int rc = head_train_check("dc_spike_head_train_bwd", a, kh, bh, y, da, grad_partial, pool, N, T, C)) return rc;
  DC_REQUIRE(dc_aligned16(da), DC_EINVAL, "dc_spike_head_train_bwd: da must be 16-byte aligned");
  const int tilesT = dc_cdiv(T, HEADT_BTT);
  const float inv_count = (float)(1.0 / ((double)N * (double)T));
  hipLaunchKernelGGL(spike_head_train_bwd_kernel, dim3((unsigned)(N * tilesT)), dim3(256), 0, (hipStream_t)stream, a, kh, bh, pool,
                     y, wpos, wneg, inv_count, da, grad_partial, T, C, tilesT);
  DC_CHECK_LAUNCH("dc_spike_head_train_bwd");
  return DC_OK;
}
