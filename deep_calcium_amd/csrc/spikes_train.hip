// UNet1D training (deepcalcium/models/spikes/unet_1d_segmentation.py: unet1d :49-148 as fit :217-380 trains it), gfx950:
// the 1-D hot path of a train step that spikes.hip (inference) and elementwise.hip (BatchNorm / ReLU / Dropout / Adam on
// [pixels][C] tensors, pixels = N * T) do not already cover.
//   dc_conv1d_stats              per-channel (sum, sumsq) of the pre-BatchNorm output, double partials
//   dc_conv1d_k5_wgrad           dw of Conv1D(nbf, 5, 'same'): wgrad.hip, wgrad_kernel<1, 5, ...>
//   dc_conv1d_k5_c1_wgrad        the same for the 1-channel first layer (vector kernel)
//   dc_maxpool1d_2_bwd           MaxPooling1D(2) backward (argmax recomputed, first maximum wins) + the skip gradient
//   dc_upsample1d_2x_drop_fwd/_bwd   UpSampling1D + Dropout (:114-115): spikes.hip, beside the inference up-sampling
//   dc_spike_head_train_fwd/_bwd     the head (:139-145) with the weighted loss and the metric sums (utils/spikes.py:11-57)
// The data gradient of a conv_layer is dc_conv1d_k5_fwd on dz with the kernel packed flipped and transposed (dcunet.h).
// Conventions of spikes.hip: channels-last fp32, nothing is read across a trace boundary, fp32 (or double) accumulation in a
// FIXED order and no atomics -- a repeated call gives the same bits.
#include "spikes_common.h"

// ---------------------------------------------------------------------------------------------------------------------
// BatchNorm statistics of z [pixels][C] (sample stride z_ld): partial[block][C][2] = (sum z, sum z^2) in DOUBLE, the layout
// dc_bn_stats_finalize reads with groups == 1.  256 threads = PPB sample lanes x C/4 channel quads (threads past PPB * C4
// idle); a thread adds its samples in ascending order, the sample lanes of a quad are added in lane order by lane 0.
#define STATS_MAX_BLOCKS 1024
#define STATS_SAMPLES_PER_LANE 16

__global__ __launch_bounds__(256) void conv1d_stats_kernel(const float* __restrict__ z, long z_ld, double* __restrict__ partial,
                                                           long pixels, int C) {
  const int C4 = C >> 2, PPB = 256 / C4;
  const int tid = threadIdx.x, q = tid % C4, pl = tid / C4;
  double s[8] = {0., 0., 0., 0., 0., 0., 0., 0.};       // (sum z, sum z^2) of the quad's 4 channels: s[e], s[4 + e]
  if (pl < PPB) {
    for (long pix = (long)blockIdx.x * PPB + pl; pix < pixels; pix += (long)gridDim.x * PPB) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(z + pix * z_ld + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double d = (double)v[e];
        s[e] += d;
        s[4 + e] += d * d;
      }
    }
  }
  quad_lane_sum(s, C4, PPB, q, pl);
  if (pl == 0) {
    double* dst = partial + ((long)blockIdx.x * C + 4 * q) * 2;
#pragma unroll
    for (int e = 0; e < 4; ++e) { dst[2 * e] = s[e]; dst[2 * e + 1] = s[4 + e]; }
  }
}

static int stats_blocks(long pixels, int C) { return quad_blocks(pixels, C, STATS_SAMPLES_PER_LANE, STATS_MAX_BLOCKS); }

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
// First layer (Cin == 1): dw[tap][0][co] = sum over (n, t) of x[n][t + tap - 2] * dz[n][t][co]; x is the (N, T) trace matrix.
// 256 threads = PPB sample lanes x Cout/4 channel quads; a thread walks its samples s = n * T + t in ascending order with
// 20 fmaf accumulators (5 taps x 4 channels), the lanes of a quad are added in lane order, one slab per workgroup, the slabs
// by dc_reduce_partials.
#define C1W_MAX_BLOCKS 512
#define C1W_SAMPLES_PER_LANE 32

__global__ __launch_bounds__(256) void conv1d_c1_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dz,
                                                              float* __restrict__ slabs, int T, long total, int Cout) {
  const int C4 = Cout >> 2, PPB = 256 / C4;
  const int tid = threadIdx.x, q = tid % C4, pl = tid / C4;
  float acc[20];                            // [tap][4 channels]
#pragma unroll
  for (int k = 0; k < 20; ++k) acc[k] = 0.f;
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
        for (int e = 0; e < 4; ++e) acc[tap * 4 + e] = __builtin_fmaf(xv, g[e], acc[tap * 4 + e]);
      }
    }
  }
  quad_lane_sum(acc, C4, PPB, q, pl);
  if (pl == 0) {
    float* dst = slabs + (long)blockIdx.x * 5 * Cout + 4 * q;
#pragma unroll
    for (int tap = 0; tap < 5; ++tap)
#pragma unroll
      for (int e = 0; e < 4; ++e) dst[tap * Cout + e] = acc[tap * 4 + e];
  }
}

static int c1w_blocks(long total, int Cout) { return quad_blocks(total, Cout, C1W_SAMPLES_PER_LANE, C1W_MAX_BLOCKS); }

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
  if (int rc = spikes_check_shape("dc_maxpool1d_2_bwd", N, T, "C", C, "in_ld", in_ld)) return rc;
  if (int rc = spikes_check_ld("dc_maxpool1d_2_bwd", "dx_ld", dx_ld, "C", C)) return rc;
  if (skip)
    if (int rc = spikes_check_ld("dc_maxpool1d_2_bwd", "skip_ld", skip_ld, "C", C)) return rc;
  const int Tp = (T + 1) / 2;
  const long total = (long)N * Tp * (C / 4);
  hipLaunchKernelGGL(maxpool1d_2_bwd_kernel, dim3(spikes_blocks(total)), dim3(256), 0, (hipStream_t)stream, dy, in, in_ld, skip,
                     skip_ld, dx, dx_ld, T, Tp, C / 4, total);
  DC_CHECK_LAUNCH("dc_maxpool1d_2_bwd");
  return DC_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The head in training (spikes_common.h).  The forward is spike_head_fwd_kernel<true>: the inference kernel's own body, so p is
// the same bits, plus the weighted loss and the metric sums; the backward below forms p from the same pieces.
//
// Backward.  dp = dl/dp / (N * T); dm1 = dp * p * q; dm0 = -dm1; each dm_j[t] goes to the FIRST maximal logit of t's window,
// written as a gather so that no atomics are needed:  dl_j[s] = sum over t in [s - pool/2, s + (pool-1)/2] with
// argmax_j(t) == s of dm_j[t], in ascending t.  Then da[s][c] = dl_0[s] kh[c][0] + dl_1[s] kh[c][1], and the block's share
// of the head's own gradient: grad_partial[block][2C + 2] = (dkh[c][j] = sum_s a[s][c] dl_j[s] ..., dbh[j] = sum_s dl_j[s]),
// both in ascending s -- the flat (kernel, bias) order, so dc_reduce_partials over the blocks yields the two arrays.
// A workgroup owns HEAD_BTT samples s and needs the logits of s +- (pool - 1): the window of every t whose window holds s.
__global__ __launch_bounds__(256) void spike_head_train_bwd_kernel(const float* __restrict__ a, const float* __restrict__ kh,
                                                                   const float* __restrict__ bh, int pool,
                                                                   const uint8_t* __restrict__ y, float wpos, float wneg,
                                                                   float inv_count, float* __restrict__ da,
                                                                   float* __restrict__ grad_partial, int T, int C, int tilesT) {
  __shared__ float l0[256], l1[256];
  __shared__ float dm[256];          // dm1 of sample t = tbase + index
  __shared__ int am0[256], am1[256]; // first argmax (absolute sample) of each logit channel over t's window
  __shared__ float dl0[HEAD_BTT], dl1[HEAD_BTT];
  const int trace = blockIdx.x / tilesT;
  const int t0 = (blockIdx.x - trace * tilesT) * HEAD_BTT;
  const int left = (pool - 1) / 2, right = pool / 2;
  const int tid = threadIdx.x;
  const int ubase = t0 - (pool - 1);          // first sample whose logits are formed
  const int tbase = t0 - right;               // first t whose window can hold a sample of this tile
  {
    const int u = ubase + tid;
    if (tid < HEAD_BTT + 2 * (pool - 1) && u >= 0 && u < T) {
      float s0, s1;
      head_logits(a + ((long)trace * T + u) * C, kh, bh, C, s0, s1);
      l0[tid] = s0;
      l1[tid] = s1;
    }
  }
  __syncthreads();
  {
    const int t = tbase + tid;
    if (tid < HEAD_BTT + pool - 1 && t >= 0 && t < T) {
      int lo, hi, i0, i1;
      float m0, m1, pv, qv;
      head_window(t, pool, T, lo, hi);                                 // inside [ubase, ubase + BTT + 2 (pool - 1))
      head_window_max(l0, l1, ubase, lo, hi, m0, m1, i0, i1);
      head_pq(m0, m1, pv, qv);
      const bool pos = y[(long)trace * T + t] != 0;
      const float dldp = pos ? -wpos / (pv + 1e-7f) : wneg / (qv + 1e-7f);
      dm[tid] = dldp * inv_count * pv * qv;
      am0[tid] = i0;
      am1[tid] = i1;
    }
  }
  __syncthreads();
  const int s = t0 + tid;
  if (tid < HEAD_BTT) {
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
  const int ns = min(HEAD_BTT, T - t0);
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
  if (int rc = spikes_check_shape(fn, N, T, "C", C)) return rc;
  DC_REQUIRE(pool >= 1 && pool <= HEAD_MAX_POOL, DC_EINVAL, "%s: pool=%d must be in 1..%d", fn, pool, HEAD_MAX_POOL);
  DC_REQUIRE((long)N * dc_cdiv(T, HEAD_BTT) < (1L << 31), DC_EUNSUP, "%s: too many workgroups", fn);
  return DC_OK;
}

extern "C" int dc_spike_head_train_fwd_blocks(int N, int T) {
  return (N < 1 || T < 1 || (long)N * dc_cdiv(T, HEAD_TT) >= (1L << 31)) ? 0 : N * dc_cdiv(T, HEAD_TT);
}
extern "C" int dc_spike_head_train_bwd_blocks(int N, int T) {
  return (N < 1 || T < 1 || (long)N * dc_cdiv(T, HEAD_BTT) >= (1L << 31)) ? 0 : N * dc_cdiv(T, HEAD_BTT);
}

extern "C" int dc_spike_head_train_fwd(const float* a, const float* kh, const float* bh, int pool, const uint8_t* y, float wpos,
                                       float wneg, float* p, float* partial, int N, int T, int C, dc_stream_t stream) {
  if (int rc = head_train_check("dc_spike_head_train_fwd", a, kh, bh, y, p, partial, pool, N, T, C)) return rc;
  const int tilesT = dc_cdiv(T, HEAD_TT);
  hipLaunchKernelGGL(spike_head_fwd_kernel<true>, dim3((unsigned)(N * tilesT)), dim3(256), 0, (hipStream_t)stream, a, kh, bh, pool,
                     y, wpos, wneg, p, partial, T, C, tilesT);
  DC_CHECK_LAUNCH("dc_spike_head_train_fwd");
  return DC_OK;
}

extern "C" int dc_spike_head_train_bwd(const float* a, const float* kh, const float* bh, int pool, const uint8_t* y, float wpos,
                                       float wneg, float* da, float* grad_partial, int N, int T, int C, dc_stream_t stream) {
  if (int rc = head_train_check("dc_spike_head_train_bwd", a, kh, bh, y, da, grad_partial, pool, N, T, C)) return rc;
  DC_REQUIRE(dc_aligned16(da), DC_EINVAL, "dc_spike_head_train_bwd: da must be 16-byte aligned");
  const int tilesT = dc_cdiv(T, HEAD_BTT);
  const float inv_count = (float)(1.0 / ((double)N * (double)T));
  hipLaunchKernelGGL(spike_head_train_bwd_kernel, dim3((unsigned)(N * tilesT)), dim3(256), 0, (hipStream_t)stream, a, kh, bh, pool,
                     y, wpos, wneg, inv_count, da, grad_partial, T, C, tilesT);
  DC_CHECK_LAUNCH("dc_spike_head_train_bwd");
  return DC_OK;
}
