// UNet1D spike inference (deepcalcium/models/spikes/unet_1d_segmentation.py:49-148, predict :422-459), gfx950.
//
// Five launches cover the graph in inference mode (Dropout is the identity):
//   dc_conv1d_k5_fwd     Conv1D(nbf, 5, 'same') + BatchNormalization + relu  (:81-84)   implicit GEMM, fp32 matrix cores
//   dc_conv1d_k5_c1_fwd  the same block on the 1-channel network input       (:86-89)   vector kernel, K = 5
//   dc_maxpool1d_2_fwd   MaxPooling1D(2, strides=2)                          (:93)
//   dc_upsample1d_2x_fwd UpSampling1D()                                      (:79)         and, in training, with Dropout:
//                        dc_upsample1d_2x_drop_fwd / _bwd                    (:114-115)
//   dc_spike_head_fwd    Conv1D(2, 1) -> MaxPooling1D(margin + 1, 1, 'same') -> softmax -> [:, :, -1]   (:139-145)
//
// Activations are channels-last fp32 [N][T][C]; a trace is one row of N and NOTHING crosses from one trace into the next:
// every workgroup of every kernel here works inside one trace, the convolution halo outside [0, T) of that trace is zero,
// and the contraction order of a sample does not depend on N or on where the trace sits in the batch -- a trace's
// probabilities are the same bits however it is batched.
#include "spikes_common.h"

// ---------------------------------------------------------------------------------------------------------------------
// Conv1D(k = 5, 'same') as an im2col-free implicit GEMM (the 1-D sibling of igemm_conv.hip, same LDS layout):
//   * a workgroup (256 threads = 4 waves) owns TT consecutive samples of ONE trace and BN output columns;
//   * per CK-channel chunk the TT + 4 samples (2-sample halo either side, zero outside the trace) are staged once into LDS
//     as [channel group g][sample][4 channels] (plane stride == 2 mod 8), the 5-tap weight slab as [tap][g][column][4 ch];
//   * the 5 taps are 5 shifted ds_read_b128 windows of the same patch (the tap folds into the read's immediate offset);
//   * fp32 accumulation in a FIXED K order: chunk, then tap, then channel -- an exact fmaf chain per output, so no fp16
//     range guard and bit-identical results for a trace in any batch;
//   * epilogue: channel on the lane (C/D col = lane & 31), so the folded-BN (scale, shift) are per-lane scalars.
template <int WAVES_M, int MB, int NB, int CK>
struct Conv1dCfg {
  static constexpr int TAPS = 5, PAD = 2;
  static constexpr int WAVES_N = 4 / WAVES_M;
  static constexpr int TT = WAVES_M * MB * 32;
  static constexpr int BN = WAVES_N * NB * 32;
  static constexpr int NH = TT + TAPS - 1;                 // staged samples
  static constexpr int PS = ((NH + 5) / 8) * 8 + 2;        // plane stride == 2 (mod 8): ds_write_b128 conflict-free
  static constexpr int G = CK / 4;
  static constexpr int NA = (NH * G + 255) / 256;
  static constexpr int NBV = (TAPS * G * BN + 255) / 256;
  static constexpr int LDS_SLOTS = G * PS + TAPS * G * BN;
  static_assert(G % 2 == 0, "CK must be a multiple of 8");
  static_assert(256 % G == 0 && 256 % BN == 0, "staging assumes G and BN divide the block size");
  static_assert(LDS_SLOTS * 16 <= 32 * 1024, "two workgroups per CU with room to spare");
};

struct Conv1dParams {
  const float* in;      // [N][T][Cin] dense
  const float* wp;      // dc_pack_weights(taps 5): [tap][Cin/4][Cout][4]
  const float* scale;   // [Cout]
  const float* shift;   // [Cout]
  float* out;           // sample stride outLd
  long outLd;
  int N, T, Cin, Cout;
  int tilesT;
  int relu;
};

template <int WAVES_M, int MB, int NB, int CK>
__global__ __launch_bounds__(256, 2) void conv1d_k5_kernel(Conv1dParams p) {
  using Cfg = Conv1dCfg<WAVES_M, MB, NB, CK>;
  constexpr int TAPS = Cfg::TAPS, TT = Cfg::TT, BN = Cfg::BN, NH = Cfg::NH;
  constexpr int PS = Cfg::PS, G = Cfg::G, NA = Cfg::NA, NBV = Cfg::NBV;

  __shared__ f32x4 lds[Cfg::LDS_SLOTS];
  f32x4* ldsA = lds;
  f32x4* ldsB = lds + G * PS;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, h = lane >> 5;
  const int wave_m = wave % WAVES_M, wave_n = wave / WAVES_M;

  // XCD-aware rasterisation (common.h dc_xcd_first): column block fastest, so the workgroups that re-read one time tile for
  // different output columns run back to back on one L2.  Speed only; bijective for every grid size.
  const int nblk = (p.Cout + BN - 1) / BN;
  const int work = dc_xcd_first(blockIdx.x, (int)gridDim.x);
  const int tile_id = work / nblk;
  const int tt = tile_id % p.tilesT;
  const int trace = tile_id / p.tilesT;
  const int n0 = (work - tile_id * nblk) * BN;
  const int t0 = tt * TT;
  const int Cin4 = p.Cin >> 2;

  const f32x4* in4 = reinterpret_cast<const f32x4*>(p.in) + (long)trace * p.T * Cin4;
  const f32x4* wp4 = reinterpret_cast<const f32x4*>(p.wp);

  // chunk-invariant staging coordinates: G and BN divide 256, so a thread's channel group / column never change
  constexpr int A_STEP = 256 / G;
  constexpr int B_STEP = 256 / BN;
  const int a_g = tid % G, a_s0 = tid / G;
  const int b_j = tid % BN, b_row0 = tid / BN;
  const bool b_col_ok = n0 + b_j < p.Cout;
  int a_goff[NA];       // float4 offset inside THIS trace (channel group 0 of the chunk); -1 = zero (halo outside [0, T))
#pragma unroll
  for (int it = 0; it < NA; ++it) {
    const int s = a_s0 + it * A_STEP;
    const int t = t0 - Cfg::PAD + s;
    a_goff[it] = (s < NH && t >= 0 && t < p.T) ? (t * Cin4 + a_g) : -1;
  }

  f32x4 ra[NA], rb[NBV];
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  auto load_chunk = [&](int c0) {
    const int cg0 = c0 >> 2;
    const bool a_ch_ok = (cg0 + a_g) < Cin4;
#pragma unroll
    for (int it = 0; it < NA; ++it) ra[it] = (a_goff[it] >= 0 && a_ch_ok) ? in4[a_goff[it] + cg0] : zero4;
#pragma unroll
    for (int it = 0; it < NBV; ++it) {
      const int row = b_row0 + it * B_STEP;
      const int tap = row / G, g = row - tap * G;
      const bool ok = b_col_ok && row < TAPS * G && (cg0 + g) < Cin4;
      rb[it] = ok ? wp4[(long)(tap * Cin4 + cg0 + g) * p.Cout + n0 + b_j] : zero4;
    }
  };

  int a_base[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) a_base[mb] = h * PS + (wave_m * MB + mb) * 32 + li;
  const int b_base = h * BN + wave_n * NB * 32 + li;

  f32x16 acc[MB][NB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.f;

  load_chunk(0);
  for (int c0 = 0; c0 < p.Cin; c0 += CK) {
#pragma unroll
    for (int it = 0; it < NA; ++it) {
      const int s = a_s0 + it * A_STEP;
      if (s < NH) ldsA[a_g * PS + s] = ra[it];
    }
#pragma unroll
    for (int it = 0; it < NBV; ++it) {
      const int row = b_row0 + it * B_STEP;
      if (row < TAPS * G) ldsB[row * BN + b_j] = rb[it];
    }
    __syncthreads();
    if (c0 + CK < p.Cin) load_chunk(c0 + CK);   // in flight behind the MFMA block below

#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap) {
#pragma unroll
      for (int g2 = 0; g2 < G / 2; ++g2) {
        f32x4 a[MB], b[NB];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) a[mb] = ldsA[a_base[mb] + 2 * g2 * PS + tap];
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) b[nb] = ldsB[b_base + (tap * G + 2 * g2) * BN + nb * 32];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb)
              acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mb][e], b[nb][e], acc[mb][nb], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // C/D map of the 32x32 MFMA: col = lane & 31 (column n), row = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) (sample m)
  float* out = p.out + (long)trace * p.T * p.outLd;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int n = n0 + (wave_n * NB + nb) * 32 + li;
    const bool n_ok = n < p.Cout;
    const float sc = n_ok ? p.scale[n] : 1.f;
    const float sh = n_ok ? p.shift[n] : 0.f;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int t = t0 + (wave_m * MB + mb) * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
        if (n_ok && t < p.T) {
          float v = __builtin_fmaf(acc[mb][nb][r], sc, sh);
          if (p.relu) v = fmaxf(v, 0.f);
          out[(long)t * p.outLd + n] = v;
        }
      }
    }
  }
}

// Tile shape: 128 samples x 64 columns, CK = 16 (29.3 KB of LDS).  One shape for every layer: the routing then depends on
// nothing, and a trace's contraction order is the same wherever it runs.
#define CONV1D_CFG 4, 1, 2, 16

static int conv1d_check(const char* fn, const void* x, const void* w, const void* scale, const void* shift, const void* y,
                        long y_ld, int N, int T, int Cin, int Cout) {
  DC_REQUIRE(x && w && scale && shift && y, DC_EINVAL, "%s: null pointer", fn);
  DC_REQUIRE(dc_aligned16(x) && dc_aligned16(w) && dc_aligned16(y), DC_EINVAL, "%s: pointers must be 16-byte aligned", fn);
  if (int rc = spikes_check_shape(fn, N, T, "Cout", Cout, "y_ld", y_ld, Cin >= 1)) return rc;
  DC_REQUIRE((long)T * Cin < (1L << 31) && (long)T * y_ld < (1L << 31), DC_EUNSUP, "%s: one trace exceeds 2^31 elements", fn);
  return DC_OK;
}

extern "C" int dc_conv1d_k5_fwd(const float* x, const float* wp, const float* scale, const float* shift, int relu, float* y,
                                long y_ld, int N, int T, int Cin, int Cout, dc_stream_t stream) {
  if (int rc = conv1d_check("dc_conv1d_k5_fwd", x, wp, scale, shift, y, y_ld, N, T, Cin, Cout)) return rc;
  DC_REQUIRE(Cin % 4 == 0, DC_EINVAL, "dc_conv1d_k5_fwd: Cin=%d must be a multiple of 4", Cin);
  using Cfg = Conv1dCfg<CONV1D_CFG>;
  Conv1dParams p{};
  p.in = x; p.wp = wp; p.scale = scale; p.shift = shift; p.out = y; p.outLd = y_ld;
  p.N = N; p.T = T; p.Cin = Cin; p.Cout = Cout; p.relu = relu;
  p.tilesT = dc_cdiv(T, Cfg::TT);
  const long grid = (long)N * p.tilesT * dc_cdiv(Cout, Cfg::BN);
  DC_REQUIRE(grid < (1L << 31), DC_EUNSUP, "dc_conv1d_k5_fwd: %ld workgroups", grid);
  hipLaunchKernelGGL((conv1d_k5_kernel<CONV1D_CFG>), dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, p);
  DC_CHECK_LAUNCH("dc_conv1d_k5_fwd");
  return DC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// First layer, Cin == 1 (:86-89: expand_dims + conv_layer): K = 5, memory-bound -- one thread per (sample, 4 channels),
// the five taps an fmaf chain in tap order, the trace itself read through L1 (5 overlapping reads per sample).
__global__ __launch_bounds__(256) void conv1d_k5_c1_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                           const float* __restrict__ scale, const float* __restrict__ shift,
                                                           int relu, float* __restrict__ y, long y_ld, int T, int C4, long total) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cg = (int)(i % C4);
    const long s = i / C4;            // n * T + t
    const int t = (int)(s % T);
    const float* xr = x + (s - t);    // this trace
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < 5; ++tap) {
      const int u = t + tap - 2;
      const float xv = (u >= 0 && u < T) ? xr[u] : 0.f;
      const f32x4 wv = reinterpret_cast<const f32x4*>(w)[tap * C4 + cg];
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(xv, wv[e], acc[e]);
    }
    const f32x4 sc = reinterpret_cast<const f32x4*>(scale)[cg], sh = reinterpret_cast<const f32x4*>(shift)[cg];
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = __builtin_fmaf(acc[e], sc[e], sh[e]);
      if (relu) v[e] = fmaxf(v[e], 0.f);
    }
    *reinterpret_cast<f32x4*>(y + s * y_ld + 4 * cg) = v;
  }
}

extern "C" int dc_conv1d_k5_c1_fwd(const float* x, const float* w, const float* scale, const float* shift, int relu, float* y,
                                   long y_ld, int N, int T, int Cout, dc_stream_t stream) {
  if (int rc = conv1d_check("dc_conv1d_k5_c1_fwd", w, w, scale, shift, y, y_ld, N, T, 1, Cout)) return rc;
  DC_REQUIRE(x, DC_EINVAL, "dc_conv1d_k5_c1_fwd: null pointer");
  DC_REQUIRE(dc_aligned16(scale) && dc_aligned16(shift), DC_EINVAL, "dc_conv1d_k5_c1_fwd: scale / shift must be 16-byte aligned");
  const long total = (long)N * T * (Cout / 4);
  hipLaunchKernelGGL(conv1d_k5_c1_kernel, dim3(spikes_blocks(total)), dim3(256), 0, (hipStream_t)stream, x, w, scale, shift,
                     relu, y, y_ld, T, Cout / 4, total);
  DC_CHECK_LAUNCH("dc_conv1d_k5_c1_fwd");
  return DC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// MaxPooling1D(2, strides=2), 'valid' (:93): out[n][t][c] = max(in[n][2t][c], in[n][2t+1][c]), t < T / 2 (an odd last
// sample is dropped).  `in` is usually the skip slice of a concat buffer (sample stride in_ld).  Bit-exact.
__global__ __launch_bounds__(256) void maxpool1d_2_kernel(const float* __restrict__ in, long in_ld, float* __restrict__ out,
                                                          int T, int To, int C4, long total) {
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int cg = (int)(i % C4);
    const long s = i / C4;            // n * To + t
    const long n = s / To;
    const int t = (int)(s - n * To);
    const float* src = in + (n * T + 2 * t) * in_ld + 4 * cg;
    const f32x4 a = *reinterpret_cast<const f32x4*>(src), b = *reinterpret_cast<const f32x4*>(src + in_ld);
    f32x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaxf(a[e], b[e]);
    reinterpret_cast<f32x4*>(out)[i] = v;
  }
}

extern "C" int dc_maxpool1d_2_fwd(const float* in, long in_ld, float* out, int N, int T, int C, dc_stream_t stream) {
  DC_REQUIRE(in && out, DC_EINVAL, "dc_maxpool1d_2_fwd: null pointer");
  DC_REQUIRE(dc_aligned16(in) && dc_aligned16(out), DC_EINVAL, "dc_maxpool1d_2_fwd: pointers must be 16-byte aligned");
  if (int rc = spikes_check_shape("dc_maxpool1d_2_fwd", N, T, "C", C, "in_ld", in_ld)) return rc;
  const int To = T / 2;
  if (To == 0) return DC_OK;          // T == 1: the output is empty, nothing is launched
  const long total = (long)N * To * (C / 4);
  hipLaunchKernelGGL(maxpool1d_2_kernel, dim3(spikes_blocks(total)), dim3(256), 0, (hipStream_t)stream, in, in_ld, out, T, To,
                     C / 4, total);
  DC_CHECK_LAUNCH("dc_maxpool1d_2_fwd");
  return DC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// UpSampling1D() (:79), in training followed by Dropout (:114-115 and the three decoder levels after it):
//   out[n][2t][c] = in[n][t][c] * f[n][2t][c],  out[n][2t+1][c] = in[n][t][c] * f[n][2t+1][c],  f = keep-mask / keep,
// written into the first C channels of the concat buffer the next conv_layer reads (sample stride out_ld; the skip connection
// already sits behind them).  The dropout element index is that of the DENSE up-sampled tensor [N][2T][C]
// (elem = (n * 2T + u) * C + c), mask / seed conventions of dc_bn_relu_drop_fwd.  keep == 1 (inference: dc_upsample1d_2x_fwd
// launches the same kernel) reads no mask, draws nothing and moves the values bit-exact.
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
    const long s = i / C4;            // n * T + t: output samples 2s and 2s + 1 (2 * (n * T + t) = n * 2T + 2t)
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

extern "C" int dc_upsample1d_2x_fwd(const float* in, float* out, long out_ld, int N, int T, int C, dc_stream_t stream) {
  DC_REQUIRE(in && out, DC_EINVAL, "dc_upsample1d_2x_fwd: null pointer");
  DC_REQUIRE(dc_aligned16(in) && dc_aligned16(out), DC_EINVAL, "dc_upsample1d_2x_fwd: pointers must be 16-byte aligned");
  if (int rc = spikes_check_shape("dc_upsample1d_2x_fwd", N, T, "C", C, "out_ld", out_ld)) return rc;
  const long total = (long)N * T * (C / 4);
  hipLaunchKernelGGL(upsample1d_2x_drop_fwd_kernel, dim3(spikes_blocks(total)), dim3(256), 0, (hipStream_t)stream, in, out, out_ld,
                     (const uint8_t*)nullptr, 1.f, (uint64_t)0, C / 4, total);
  DC_CHECK_LAUNCH("dc_upsample1d_2x_fwd");
  return DC_OK;
}

static int up1d_check(const char* fn, const void* a, const void* b, const void* mask, long ld, float keep, int N, int T, int C) {
  DC_REQUIRE(a && b, DC_EINVAL, "%s: null pointer", fn);
  DC_REQUIRE(dc_aligned16(a) && dc_aligned16(b) && (((uintptr_t)mask) & 3) == 0, DC_EINVAL,
             "%s: tensors must be 16-byte aligned, the mask 4-byte aligned", fn);
  if (int rc = spikes_check_shape(fn, N, T, "C", C, "ld", ld)) return rc;
  DC_REQUIRE(keep > 0.f, DC_EINVAL, "%s: keep=%g must be > 0", fn, (double)keep);
  return DC_OK;
}

extern "C" int dc_upsample1d_2x_drop_fwd(const float* in, float* out, long out_ld, const uint8_t* mask, float keep, uint64_t seed,
                                         int N, int T, int C, dc_stream_t stream) {
  if (int rc = up1d_check("dc_upsample1d_2x_drop_fwd", in, out, mask, out_ld, keep, N, T, C)) return rc;
  const long total = (long)N * T * (C / 4);
  hipLaunchKernelGGL(upsample1d_2x_drop_fwd_kernel, dim3(spikes_blocks(total)), dim3(256), 0, (hipStream_t)stream, in, out, out_ld,
                     mask, keep, seed, C / 4, total);
  DC_CHECK_LAUNCH("dc_upsample1d_2x_drop_fwd");
  return DC_OK;
}

extern "C" int dc_upsample1d_2x_drop_bwd(const float* dout, long dout_ld, const uint8_t* mask, float keep, uint64_t seed,
                                         float* din, int N, int T, int C, dc_stream_t stream) {
  if (int rc = up1d_check("dc_upsample1d_2x_drop_bwd", dout, din, mask, dout_ld, keep, N, T, C)) return rc;
  const long total = (long)N * T * (C / 4);
  hipLaunchKernelGGL(upsample1d_2x_drop_bwd_kernel, dim3(spikes_blocks(total)), dim3(256), 0, (hipStream_t)stream, dout, dout_ld,
                     mask, keep, seed, din, C / 4, total);
  DC_CHECK_LAUNCH("dc_upsample1d_2x_drop_bwd");
  return DC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The head (:139-145) in one kernel, spike_head_fwd_kernel<false> of spikes_common.h: logits, 'SAME' window maximum, p.
extern "C" int dc_spike_head_fwd(const float* a, const float* kh, const float* bh, int pool, float* p, int N, int T, int C,
                                 dc_stream_t stream) {
  DC_REQUIRE(a && kh && bh && p, DC_EINVAL, "dc_spike_head_fwd: null pointer");
  DC_REQUIRE(dc_aligned16(a), DC_EINVAL, "dc_spike_head_fwd: a must be 16-byte aligned");
  if (int rc = spikes_check_shape("dc_spike_head_fwd", N, T, "C", C)) return rc;
  DC_REQUIRE(pool >= 1 && pool <= HEAD_MAX_POOL, DC_EINVAL, "dc_spike_head_fwd: pool=%d must be in 1..%d", pool, HEAD_MAX_POOL);
  const int tilesT = dc_cdiv(T, HEAD_TT);
  const long grid = (long)N * tilesT;
  DC_REQUIRE(grid < (1L << 31), DC_EUNSUP, "dc_spike_head_fwd: %ld workgroups", grid);
  hipLaunchKernelGGL(spike_head_fwd_kernel<false>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a, kh, bh, pool,
                     (const uint8_t*)nullptr, 0.f, 0.f, p, (float*)nullptr, T, C, tilesT);
  DC_CHECK_LAUNCH("dc_spike_head_fwd");
  return DC_OK;
}
