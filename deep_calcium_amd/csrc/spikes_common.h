// Shared by the UNet1D entry points (spikes.hip, spikes_train.hip): the argument
// checks they repeat, the grid-size helpers, the quad reduction of the two vector reductions, and the ONE definition of the
// head's arithmetic that the inference forward, the training forward and the training backward all use.
#pragma once
#include "common.h"

// ---- argument checks ----------------------------------------------------------------------------------------------------
// A sample stride: at least the C channels it carries, and a multiple of 4 (every access is a float4).
static inline int spikes_check_ld(const char* fn, const char* ldname, long ld, const char* cname, int C) {
  DC_REQUIRE(ld >= C && ld % 4 == 0, DC_EINVAL, "%s: %s=%ld must be a multiple of 4 and >= %s=%d", fn, ldname, ld, cname, C);
  return DC_OK;
}

// N, T >= 1; C (the caller calls it `cname`) a positive multiple of 4 -- `c_also` is whatever else the caller wants reported
// with C --; and, where there is one, the sample stride `ldname`.
static inline int spikes_check_shape(const char* fn, int N, int T, const char* cname, int C, const char* ldname = nullptr,
                                     long ld = 0, bool c_also = true) {
  DC_REQUIRE(N >= 1 && T >= 1, DC_EINVAL, "%s: N=%d and T=%d must be >= 1", fn, N, T);
  DC_REQUIRE(c_also && C >= 4 && C % 4 == 0, DC_EINVAL, "%s: %s=%d must be a positive multiple of 4", fn, cname, C);
  return ldname ? spikes_check_ld(fn, ldname, ld, cname, C) : DC_OK;
}

// ---- grid sizes ---------------------------------------------------------------------------------------------------------
// grid-stride kernels: one thread per element, at most `cap` workgroups of 256
static inline int spikes_blocks(long total, int cap = 8192) {
  const long b = (total + 255) / 256;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// quad-reduction kernels (below): 256 / (C / 4) sample lanes per workgroup, `per_lane` samples each, at most `cap` workgroups
static inline int quad_blocks(long samples, int C, int per_lane, int cap) {
  const long per_block = (long)(256 / (C / 4)) * per_lane;
  const long b = (samples + per_block - 1) / per_block;
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}

// ---- quad reduction -----------------------------------------------------------------------------------------------------
// 256 threads = PPB sample lanes x C4 channel quads (tid = pl * C4 + q; threads past PPB * C4 idle, their v all zero): K values
// per thread, added over the sample lanes of a quad IN LANE ORDER by lane 0 -- on return the threads with pl == 0 hold the
// workgroup's sums.  Call it once per kernel, from uniform control flow.
template <typename V, int K>
__device__ __forceinline__ void quad_lane_sum(V (&v)[K], int C4, int PPB, int q, int pl) {
  __shared__ V sm[256][K];
#pragma unroll
  for (int k = 0; k < K; ++k) sm[threadIdx.x][k] = v[k];
  __syncthreads();
  if (pl == 0) {
    for (int l = 1; l < PPB; ++l)
#pragma unroll
      for (int k = 0; k < K; ++k) v[k] += sm[l * C4 + q][k];
  }
}

// ---- the head (unet_1d_segmentation.py:139-145) ---------------------------------------------------------------------------
//   logits l[t][j] = bh[j] + sum_c a[t][c] kh[c][j]                           an fmaf chain in channel order
//   m[t][j] = max l[max(0, t - (pool-1)/2) ... min(T-1, t + pool/2)][j]       MaxPooling1D(pool, 1, 'same'): the SMALLER pad is
//   p[t]    = 1 / (1 + exp(m[t][0] - m[t][1]))                                on the left, and padding never wins the max
// Every kernel that needs p forms it through these four pieces, so the inference and the training probabilities are the
// same bits by construction.
#define HEAD_TT 192           // forward: output samples per workgroup (+ up to 63 of window reach = 255 logits, one per thread)
#define HEAD_BTT 128          // backward: + 2 * 63 of reach = 254 logits
#define HEAD_MAX_POOL 64
#define HEAD_SUMS 8

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

// the 'SAME' window of sample t, clipped to the trace
__device__ __forceinline__ void head_window(int t, int pool, int T, int& lo, int& hi) {
  lo = max(0, t - (pool - 1) / 2);
  hi = min(T - 1, t + pool / 2);
}

// Maxima of the two logit channels over samples [lo, hi]; l0 / l1 hold the logit of sample `base` at index 0.  i0 / i1: the
// FIRST sample that attains each maximum (strict >; the backward routes the gradient there, the forwards ignore them).
__device__ __forceinline__ void head_window_max(const float* l0, const float* l1, int base, int lo, int hi, float& m0, float& m1,
                                                int& i0, int& i1) {
  m0 = l0[lo - base];
  m1 = l1[lo - base];
  i0 = i1 = lo;
  for (int w = lo + 1; w <= hi; ++w) {
    const float c0 = l0[w - base], c1 = l1[w - base];
    if (c0 > m0) i0 = w;
    if (c1 > m1) i1 = w;
    m0 = fmaxf(m0, c0);
    m1 = fmaxf(m1, c1);
  }
}

// p and q = 1 - p, both from d = m0 - m1 (q not by subtraction: it keeps its digits where p rounds to 1)
__device__ __forceinline__ void head_pq(float m0, float m1, float& p, float& q) {
  const float d = m0 - m1;
  p = 1.f / (1.f + expf(d));
  q = 1.f / (1.f + expf(-d));
}

// The head's forward.  A workgroup owns HEAD_TT output samples of one trace and computes the logits of those plus the window's
// reach on either side into LDS (at most HEAD_TT + 63 <= 256 samples: one per thread); the window never leaves the trace.
// TRAIN (dc_spike_head_train_fwd) adds, per sample, the weighted loss and the metric terms (utils/spikes.py:11-57)
//   loss  l = -(wpos * y * log(p + 1e-7) + wneg * (1 - y) * log(q + 1e-7))
//   sums  {l, round(p) * y, round(p), clip(y - round(p), 0, 1), y}            round half to even
// and their block sums, a fixed tree over the workgroup's threads: partial[block][HEAD_SUMS] (3 spare), block = trace * tiles +
// tile.  Inference (dc_spike_head_fwd) instantiates none of that: no y, no q, no reduction and no LDS for it.
template <bool TRAIN>
__global__ __launch_bounds__(256) void spike_head_fwd_kernel(const float* __restrict__ a, const float* __restrict__ kh,
                                                             const float* __restrict__ bh, int pool,
                                                             const uint8_t* __restrict__ y, float wpos, float wneg,
                                                             float* __restrict__ p, float* __restrict__ partial, int T, int C,
                                                             int tilesT) {
  __shared__ float l0[256], l1[256];
  const int trace = blockIdx.x / tilesT;
  const int t0 = (blockIdx.x - trace * tilesT) * HEAD_TT;
  const int left = (pool - 1) / 2, right = pool / 2;
  const int tid = threadIdx.x;
  const int u = t0 - left + tid;                 // the sample whose logits this thread forms
  if (tid < HEAD_TT + left + right && u >= 0 && u < T) {
    float s0, s1;
    head_logits(a + ((long)trace * T + u) * C, kh, bh, C, s0, s1);
    l0[tid] = s0;
    l1[tid] = s1;
  }
  __syncthreads();
  const int t = t0 + tid;
  float v[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  if (tid < HEAD_TT && t < T) {
    int lo, hi, i0, i1;
    float m0, m1, pv, qv;
    head_window(t, pool, T, lo, hi);
    head_window_max(l0, l1, t0 - left, lo, hi, m0, m1, i0, i1);
    head_pq(m0, m1, pv, qv);
    p[(long)trace * T + t] = pv;
    if constexpr (TRAIN) {
      const float yv = y[(long)trace * T + t] ? 1.f : 0.f;
      const float rp = rintf(pv);
      v[0] = -(wpos * yv * logf(pv + 1e-7f) + wneg * (1.f - yv) * logf(qv + 1e-7f));
      v[1] = rp * yv;
      v[2] = rp;
      v[3] = fminf(fmaxf(yv - rp, 0.f), 1.f);
      v[4] = yv;
    }
  }
  if constexpr (TRAIN) {
    __shared__ float red[5][256];
#pragma unroll
    for (int k = 0; k < 5; ++k) red[k][tid] = v[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s)
#pragma unroll
        for (int k = 0; k < 5; ++k) red[k][tid] += red[k][tid + s];
      __syncthreads();
    }
    if (tid < HEAD_SUMS) partial[(long)blockIdx.x * HEAD_SUMS + tid] = tid < 5 ? red[tid][0] : 0.f;
  }
}
