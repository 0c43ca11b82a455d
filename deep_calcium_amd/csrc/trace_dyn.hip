// Trace dynamics on the device (include/dcunet.h, "Trace dynamics: noise and AR(1) decay"): float (R,T) traces, dF/F as
// dc_trace_baseline leaves them -> the robust noise of every trace, its autocovariance at lags 0 .. lags and the AR(1) decay g
// that fits it, the one parameter dc_trace_deconv_ar1 otherwise asks the user for.  The reference has no counterpart; the
// header's definitions are the specification and csrc/trace_dyn_math.h is their arithmetic.  One 256-thread workgroup per trace:
//   the noise is two medians, found by VALUE with an 8-bit radix descent over a monotone 64-bit key of the double -- eight
//     counting passes per order statistic over the trace (d and |d - m| are recomputed from y on every pass, so there is no
//     workspace; the trace comes from L2 after the first), integer LDS atomics only, which are order-free;
//   the fold is 256 lane sums (thread j takes t = j, j + 256, ...: coalesced) and the header's tree through LDS (dc_dyn_fold_tree);
//   for the autocovariance a tile of 256 frames plus `lags` halo is staged into LDS as centred doubles: the lags + 1 shifted
//     reads of a thread are consecutive 8-byte words (lane l reads word l + shift: 32 lanes cover the 64 banks once), and every
//     thread keeps its lags + 1 lane sums in registers.
// The AR(2) coefficients ("Trace dynamics: AR(2) coefficients") are an epilogue on the xc and the noise that launch wrote: one lane
// per trace, a 2 x 2 least squares over lags rows.
// No floating-point atomics; every output word is written by one thread.  Nothing here may be contracted or reassociated: the
// pragma of trace_dyn_math.h and the per-file flag in _build.py.
#pragma clang fp contract(off)
#include <vector>

#include "common.h"
#include "trace_dyn_math.h"
#include "trace_matrix.h"

namespace {

const int kThreads = DC_DYN_LANES;           // one thread per lane of the fold
const int kWaves = kThreads / 64;
const int kGridCap = DC_TRACE_DYN_MAX_GROUPS;        // workgroups per launch: a workgroup walks traces r, r + grid, ...
const int kTabLanes = 64;                    // dc_ar1_tables: traces per workgroup, one lane per trace
const int kTabCols = 64;                     //   entries per staged tile
const int kTabPitch = kTabCols + 1;          //   lane l writes word l * 65 + k: 16 lanes, 16 distinct even banks

static_assert(DC_DYN_LANES == DC_TRACE_DYN_LANES && DC_DYN_MAX_LAGS == DC_TRACE_DYN_MAX_LAGS, "trace_dyn_math.h and dcunet.h disagree");

struct SelectShared {
  unsigned hist[256];
  unsigned wave_total[kWaves];
  unsigned bin, rank, below, count;          // the winning digit, the rank inside it, the keys below it and in it
  unsigned long long next;
};

template <typename In>
__device__ __forceinline__ uint64_t key_at(const In* __restrict__ y, long t, bool dev, double m) {
  return dc_dyn_key(dc_dyn_value((double)y[t], (double)y[t + 1], dev, m));
}

// The k-th smallest (0-based) key among the n values of frames t < n (each reads y[t] and y[t+1]: n <= T - 1), and *le = how
// many keys are <= it.  Block-cooperative: every thread calls it with the same arguments and gets the same result.
template <typename In>
__device__ uint64_t select_key(const In* __restrict__ y, long n, bool dev, double m, unsigned k, SelectShared& sh, unsigned* le) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  uint64_t prefix = 0;
  unsigned below = 0, count = 0;
  for (int shift = 56; shift >= 0; shift -= 8) {
    sh.hist[tid] = 0;
    __syncthreads();
    for (long t = tid; t < n; t += kThreads) {
      const uint64_t key = key_at(y, t, dev, m);
      if (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&sh.hist[(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    const unsigned c = sh.hist[tid];
    unsigned incl = c;                       // inclusive scan over the 256 digits: within the wave, then over the wave totals
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    if (lane == 63) sh.wave_total[wave] = incl;
    __syncthreads();
    unsigned excl = incl - c;
    for (int w = 0; w < wave; ++w) excl += sh.wave_total[w];
    if (excl <= k && k < excl + c) {         // exactly one digit holds rank k
      sh.bin = (unsigned)tid;
      sh.rank = k - excl;
      sh.below = excl;
      sh.count = c;
    }
    __syncthreads();
    prefix |= (uint64_t)sh.bin << shift;
    k = sh.rank;
    below += sh.below;
    count = sh.count;
  }
  *le = below + count;
  return prefix;
}

// the smallest key above `key` (there is one: the caller has counted)
template <typename In>
__device__ uint64_t next_key(const In* __restrict__ y, long n, bool dev, double m, uint64_t key, SelectShared& sh) {
  const int tid = threadIdx.x;
  if (tid == 0) sh.next = ~0ull;
  __syncthreads();
  unsigned long long best = ~0ull;
  for (long t = tid; t < n; t += kThreads) {
    const uint64_t k = key_at(y, t, dev, m);
    if (k > key && k < best) best = k;
  }
  if (best != ~0ull) atomicMin(&sh.next, best);
  __syncthreads();
  return sh.next;
}

template <typename In>
__device__ double median_dev(const In* __restrict__ y, long n, bool dev, double m, SelectShared& sh) {
  const unsigned k = (unsigned)((n - 1) / 2);                        // odd n: the middle; even n: the lower of the two middle ones
  unsigned le;
  const uint64_t lo = select_key(y, n, dev, m, k, sh, &le);
  if (n & 1) return dc_dyn_unkey(lo);
  const uint64_t hi = le > k + 1 ? lo : next_key(y, n, dev, m, lo, sh);      // le comes from LDS: the branch is uniform
  return dc_dyn_mid(dc_dyn_unkey(lo), dc_dyn_unkey(hi));
}

template <typename In>
__device__ double noise_dev(const In* __restrict__ y, long T, SelectShared& sh) {
  if (T < 3) return 0.0;
  const double m = median_dev(y, T - 1, false, 0.0, sh);
  return dc_dyn_sigma(median_dev(y, T - 1, true, m, sh));
}

// Frames t >= T of a row (the padding up to ld) are never read.
template <typename In>
__global__ __launch_bounds__(kThreads) void trace_noise_kernel(const In* __restrict__ y, long ld, int R, long T, double* __restrict__ sigma) {
  __shared__ SelectShared sh;
  for (long r = blockIdx.x; r < R; r += gridDim.x) {
    const double s = noise_dev(y + r * ld, T, sh);
    if (threadIdx.x == 0) sigma[r] = s;
  }
}

template <typename In>
__global__ __launch_bounds__(kThreads) void trace_ar1_estimate_kernel(const In* __restrict__ y, long ld, int R, long T, int lags,
                                                                     const double* __restrict__ sn, double* __restrict__ sigma,
                                                                     double* __restrict__ xc, double* __restrict__ g_raw) {
  __shared__ SelectShared sh;
  __shared__ double red[(DC_DYN_MAX_LAGS + 1) * kThreads];
  __shared__ double tile[kThreads + DC_DYN_MAX_LAGS];
  __shared__ double cov[DC_DYN_MAX_LAGS + 1];
  const int tid = threadIdx.x;
  for (long r = blockIdx.x; r < R; r += gridDim.x) {
    const In* __restrict__ row = y + r * ld;
    double noise = 0.0;
    if (sigma) {
      noise = noise_dev(row, T, sh);
      if (tid == 0) sigma[r] = noise;
    }
    // mean = fold(y, T) / T
    double s = 0.0;
    for (long t = tid; t < T; t += kThreads) s = s + (double)row[t];
    red[tid] = s;
    dc_dyn_fold_tree(red, 1);
    const double mean = red[0] / (double)T;
    // q_l = fold(t -> c[t] c[t + l], T - l), c = y - mean: lane sums in registers
    double acc[DC_DYN_MAX_LAGS + 1];
#pragma unroll
    for (int l = 0; l <= DC_DYN_MAX_LAGS; ++l) acc[l] = 0.0;
    for (long t0 = 0; t0 < T; t0 += kThreads) {
      __syncthreads();                                               // the previous tile (and red[0]) has been consumed
      for (int i = tid; i < kThreads + lags; i += kThreads)
        if (t0 + i < T) tile[i] = (double)row[t0 + i] - mean;
      __syncthreads();
      const long t = t0 + tid;
      if (t < T) {
        const double a = tile[tid];
#pragma unroll
        for (int l = 0; l <= DC_DYN_MAX_LAGS; ++l)
          if (l <= lags && t + l < T) acc[l] = acc[l] + a * tile[tid + l];
      }
    }
#pragma unroll
    for (int l = 0; l <= DC_DYN_MAX_LAGS; ++l)
      if (l <= lags) red[l * kThreads + tid] = acc[l];
    dc_dyn_fold_tree(red, lags + 1);
    if (tid <= lags) {
      const double v = red[tid * kThreads] / (double)T;
      cov[tid] = v;
      xc[r * (lags + 1) + tid] = v;
    }
    __syncthreads();
    if (tid == 0) g_raw[r] = dc_dyn_decay(cov, lags, sn ? sn[r] : noise, T);
    __syncthreads();                                                 // cov and red are free for the next trace
  }
}

// One wave per 64 traces, one lane per trace: a row of the table is a chain of multiplications, so a lane walks its row and the
// tile of 64 rows x 64 entries goes through LDS to be written with coalesced rows.  Rows r >= R and entries l > T are not written.
__global__ __launch_bounds__(kTabLanes) void ar1_tables_kernel(const double* __restrict__ g, int R, long T, double* __restrict__ G, long ldG) {
  __shared__ double tile[kTabLanes * kTabPitch];
  const int lane = threadIdx.x;
  const long r0 = (long)blockIdx.x * kTabLanes;
  const int rows = R - r0 < kTabLanes ? (int)(R - r0) : kTabLanes;
  const double gg = r0 + lane < R ? g[r0 + lane] : 0.0;
  double cur = 1.0;                                                  // G[l0] of this lane's row
  for (long l0 = 0; l0 <= T; l0 += kTabCols) {
    const int cols = T + 1 - l0 < kTabCols ? (int)(T + 1 - l0) : kTabCols;
    __syncthreads();                                                 // the previous tile has been written out
    for (int k = 0; k < cols; ++k) {
      tile[lane * kTabPitch + k] = cur;
      cur = cur * gg;
    }
    __syncthreads();
    if (lane < cols)
      for (int j = 0; j < rows; ++j) G[(r0 + j) * ldG + l0 + lane] = tile[j * kTabPitch + lane];
  }
}

// The per-trace epilogue of the AR(2) estimate: one lane per trace, which reads its lags + 1 covariances and its noise and writes
// its two coefficients.  Beyond the capped grid a lane walks traces r, r + lanes, ...
__global__ __launch_bounds__(kTabLanes) void trace_ar2_solve_kernel(const double* __restrict__ xc, int R, long T, int lags,
                                                                    const double* __restrict__ sn, double* __restrict__ g12_raw) {
  const long step = (long)gridDim.x * kTabLanes;
  for (long r = (long)blockIdx.x * kTabLanes + threadIdx.x; r < R; r += step) {
    double g1, g2;
    dc_dyn_ar2_solve(xc + r * (lags + 1), lags, sn[r], T, &g1, &g2);
    g12_raw[2 * r] = g1;
    g12_raw[2 * r + 1] = g2;
  }
}

// one matrix of traces: what every entry point that takes one refuses, in this order
int check_traces(const char* who, const void* y, int is_f64, long ld, int R, long T) {
  const int rc = dc_trace_check_counts(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  DC_REQUIRE(dc_trace_aligned(y, is_f64), DC_EINVAL, "%s: misaligned buffer", who);
  return dc_trace_check_limits(who, R, T);
}

int check_estimate(const char* who, int lags, const double* sn, const double* sigma, const double* xc, const double* g_raw) {
  DC_REQUIRE(xc && g_raw && (sn || sigma), DC_EINVAL, "%s: null pointer", who);
  DC_REQUIRE(dc_aligned(7, sn, sigma, xc, g_raw), DC_EINVAL, "%s: misaligned buffer", who);
  DC_REQUIRE(lags >= 1 && lags <= DC_TRACE_DYN_MAX_LAGS, DC_EINVAL, "%s: lags = %d is outside [1, %d]", who, lags, DC_TRACE_DYN_MAX_LAGS);
  return DC_OK;
}

// what both entry points of the AR(2) solve refuse, in this order: they take no matrix of traces, only its counts
int check_solve(const char* who, const double* xc, int R, long T, int lags, const double* sn, const double* g12_raw) {
  DC_REQUIRE(xc && sn && g12_raw, DC_EINVAL, "%s: null pointer", who);
  DC_REQUIRE(dc_aligned(7, xc, sn, g12_raw), DC_EINVAL, "%s: misaligned buffer", who);
  DC_REQUIRE(lags >= 2 && lags <= DC_TRACE_DYN_MAX_LAGS, DC_EINVAL, "%s: lags = %d is outside [2, %d]", who, lags, DC_TRACE_DYN_MAX_LAGS);
  DC_REQUIRE(R >= 0 && T >= 0, DC_EINVAL, "%s: negative count (R %d, T %ld)", who, R, T);
  return dc_trace_check_limits(who, R, T);
}

unsigned groups_for(int R) { return (unsigned)(R < kGridCap ? R : kGridCap); }

}  // namespace

extern "C" int dc_trace_noise(const void* y, int is_f64, long ld, int R, long T, double* sigma, dc_stream_t stream) {
  const char* who = "dc_trace_noise";
  DC_REQUIRE(sigma, DC_EINVAL, "%s: null pointer", who);
  DC_REQUIRE(dc_aligned(7, sigma), DC_EINVAL, "%s: misaligned buffer", who);
  const int rc = check_traces(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  if (R == 0 || T == 0) return DC_OK;
  if (is_f64)
    hipLaunchKernelGGL(trace_noise_kernel<double>, dim3(groups_for(R)), dim3(kThreads), 0, (hipStream_t)stream, (const double*)y, ld, R, T, sigma);
  else
    hipLaunchKernelGGL(trace_noise_kernel<float>, dim3(groups_for(R)), dim3(kThreads), 0, (hipStream_t)stream, (const float*)y, ld, R, T, sigma);
  DC_CHECK_LAUNCH(who);
  return DC_OK;
}

extern "C" int dc_trace_ar1_estimate(const void* y, int is_f64, long ld, int R, long T, int lags, const double* sn, double* sigma, double* xc,
                                     double* g_raw, dc_stream_t stream) {
  const char* who = "dc_trace_ar1_estimate";
  int rc = check_estimate(who, lags, sn, sigma, xc, g_raw);
  if (rc != DC_OK) return rc;
  rc = check_traces(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  if (R == 0 || T == 0) return DC_OK;
  if (is_f64)
    hipLaunchKernelGGL(trace_ar1_estimate_kernel<double>, dim3(groups_for(R)), dim3(kThreads), 0, (hipStream_t)stream, (const double*)y, ld, R, T,
                       lags, sn, sigma, xc, g_raw);
  else
    hipLaunchKernelGGL(trace_ar1_estimate_kernel<float>, dim3(groups_for(R)), dim3(kThreads), 0, (hipStream_t)stream, (const float*)y, ld, R, T,
                       lags, sn, sigma, xc, g_raw);
  DC_CHECK_LAUNCH(who);
  return DC_OK;
}

extern "C" int dc_ar1_tables(const double* g, int R, long T, double* G, long ldG, dc_stream_t stream) {
  const char* who = "dc_ar1_tables";
  DC_REQUIRE(g && G, DC_EINVAL, "%s: null pointer", who);
  DC_REQUIRE(dc_aligned(7, g, G), DC_EINVAL, "%s: misaligned buffer", who);
  DC_REQUIRE(R >= 0 && T >= 0, DC_EINVAL, "%s: negative count (R %d, T %ld)", who, R, T);
  DC_REQUIRE(ldG >= T + 1, DC_EINVAL, "%s: ldG = %ld is below T + 1 = %ld", who, ldG, T + 1);
  const int rc = dc_trace_check_limits(who, R, T);
  if (rc != DC_OK) return rc;
  if (R == 0) return DC_OK;                                          // T == 0 still has the entry G[r][0]
  const unsigned groups = (unsigned)(((long)R + kTabLanes - 1) / kTabLanes);                 // <= 2^25: no cap
  hipLaunchKernelGGL(ar1_tables_kernel, dim3(groups), dim3(kTabLanes), 0, (hipStream_t)stream, g, R, T, G, ldG);
  DC_CHECK_LAUNCH(who);
  return DC_OK;
}

extern "C" int dc_trace_ar1_estimate_host(const void* y, int is_f64, long ld, int R, long T, int lags, const double* sn, double* sigma,
                                          double* xc, double* g_raw) {
  const char* who = "dc_trace_ar1_estimate_host";
  int rc = check_estimate(who, lags, sn, sigma, xc, g_raw);
  if (rc != DC_OK) return rc;
  rc = check_traces(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  if (R == 0 || T == 0) return DC_OK;
  std::vector<double> buf;
  for (int r = 0; r < R; ++r) {
    double* cov = xc + (long)r * (lags + 1);
    double noise = 0.0;
    if (is_f64) {
      const double* row = (const double*)y + (long)r * ld;
      if (sigma) noise = dc_dyn_noise_host(row, T, buf);
      dc_dyn_autocov_host(row, T, lags, cov);
    } else {
      const float* row = (const float*)y + (long)r * ld;
      if (sigma) noise = dc_dyn_noise_host(row, T, buf);
      dc_dyn_autocov_host(row, T, lags, cov);
    }
    if (sigma) sigma[r] = noise;
    g_raw[r] = dc_dyn_decay(cov, lags, sn ? sn[r] : noise, T);
  }
  return DC_OK;
}

extern "C" int dc_trace_ar2_solve(const double* xc, int R, long T, int lags, const double* sn, double* g12_raw, dc_stream_t stream) {
  const char* who = "dc_trace_ar2_solve";
  const int rc = check_solve(who, xc, R, T, lags, sn, g12_raw);
  if (rc != DC_OK) return rc;
  if (R == 0) return DC_OK;
  const long want = ((long)R + kTabLanes - 1) / kTabLanes;
  const unsigned groups = (unsigned)(want < kGridCap ? want : kGridCap);
  hipLaunchKernelGGL(trace_ar2_solve_kernel, dim3(groups), dim3(kTabLanes), 0, (hipStream_t)stream, xc, R, T, lags, sn, g12_raw);
  DC_CHECK_LAUNCH(who);
  return DC_OK;
}

extern "C" int dc_trace_ar2_solve_host(const double* xc, int R, long T, int lags, const double* sn, double* g12_raw) {
  const char* who = "dc_trace_ar2_solve_host";
  const int rc = check_solve(who, xc, R, T, lags, sn, g12_raw);
  if (rc != DC_OK) return rc;
  for (long r = 0; r < R; ++r) dc_dyn_ar2_solve(xc + r * (lags + 1), lags, sn[r], T, g12_raw + 2 * r, g12_raw + 2 * r + 1);
  return DC_OK;
}
