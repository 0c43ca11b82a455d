// Spikes by deconvolution on the device (include/dcunet.h, "Spikes by deconvolution"): float (R,T) traces, dF/F as dc_trace_baseline
// leaves them -> the non-negative AR(1) calcium c and the spikes s = c[t] - g c[t-1] that fit them best, by the pool-merging
// (OASIS-style) forward pass of csrc/deconv_math.h.  The reference has no counterpart; the header's definitions are the
// specification.  A trace is a strictly sequential computation, so the forward kernel gives one LANE to a trace and the memory
// layout is the work: the traces are row-major, so a wave's lanes would read at stride ld; a tile of 64 traces x 64 frames is
// staged through LDS with coalesced row reads instead and every lane then walks its own row of the tile.  The top pool stays in
// registers; the pools below it lie in the caller's workspace as [depth][R] planes, so the lanes of a wave that stand at the
// same depth touch one line.  The noise-constrained search (csrc/deconv_search_math.h) runs that forward pass once a round, with
// the searched parameter in the device array the pass reads anyway, and between two passes one launch that folds the residual of
// the stacks and moves every trace's bracket: nothing is read back.  Nothing here may be contracted or reassociated: the pragma of
// deconv_math.h and the per-file flag in _build.py.
#pragma clang fp contract(off)
#include <vector>

#include "common.h"
#include "deconv_math.h"
#include "deconv_search_math.h"
#include "deconv_base_math.h"
#include "trace_matrix.h"

namespace {

const int kLanes = 64;                       // traces per workgroup: one wave, one lane per trace
const int kFrames = 64;                      // frames per staged tile
const int kPitch = kFrames + 1;              // elements per tile row: lane l reads word l * 65 + k, one bank each (float), two (double)
const int kFillThreads = 256;
const int kSearchThreads = DC_DYN_LANES;     // the residual: one thread per lane of the fold
const int kSearchMaxGroups = 8192;           // DC_TRACE_DECONV_SEARCH_MAX_GROUPS: beyond, a workgroup walks several traces

// The workspace: three planes of R * T 8-byte words, pool i of trace r at word i * R + r of each.
struct DeviceStack {
  double* v;
  double* w;
  int2* tl;                                  // (t0, l)
  long R, r;
  __device__ __forceinline__ DcPool load(int32_t i) const {
    const long at = (long)i * R + r;
    DcPool p;
    p.v = v[at];
    p.w = w[at];
    const int2 x = tl[at];
    p.t0 = x.x;
    p.l = x.y;
    return p;
  }
  __device__ __forceinline__ void store(int32_t i, const DcPool& p) {
    const long at = (long)i * R + r;
    v[at] = p.v;
    w[at] = p.w;
    tl[at] = make_int2(p.t0, p.l);
  }
};

// One workgroup of one wave per 64 traces.  Rows r >= R and frames t >= T of a ragged tile are neither read nor written.
// Each = false: one decay g and one table G for all traces (dc_trace_deconv_ar1).  Each = true: trace r has the decay gs[r] and
// the table row G + r * ldG (dc_trace_deconv_ar1_each); the arithmetic of a trace is the same, only where its g and G come from.
// Base = true: the baseline base[r] leaves every frame of trace r before the penalty's shift (csrc/deconv_base_math.h).
template <typename In, bool Each, bool Base>
__global__ __launch_bounds__(kLanes) void deconv_forward_kernel(const In* __restrict__ y, long ld, int R, long T, double g_all,
                                                               const double* __restrict__ gs, const double* __restrict__ G_all, long ldG,
                                                               const double* __restrict__ lam, const double* __restrict__ smin,
                                                               const double* __restrict__ base, double* ws, int* __restrict__ pools) {
  __shared__ In tile[kLanes * kPitch];
  const int lane = threadIdx.x;
  const long r0 = (long)blockIdx.x * kLanes;
  const long r = r0 + lane;
  const bool mine = r < R;
  const int rows = R - r0 < kLanes ? (int)(R - r0) : kLanes;
  const long plane = (long)R * T;
  DeviceStack st = {ws, ws + plane, reinterpret_cast<int2*>(ws + 2 * plane), (long)R, r};
  const double la = mine ? lam[r] : 0.0, sm = mine ? smin[r] : 0.0;
  const double g = Each ? (mine ? gs[r] : 0.5) : g_all;
  const double* __restrict__ G = Each && mine ? G_all + r * ldG : G_all;
  const double b = Base && mine ? base[r] : 0.0;
  DcPool top = dc_deconv_new(0.0, 0);
  int32_t n = 0;
  for (long f0 = 0; f0 < T; f0 += kFrames) {
    const int frames = T - f0 < kFrames ? (int)(T - f0) : kFrames;
    __syncthreads();                                                 // the previous tile has been consumed
    if (lane < frames) {
#pragma unroll 8
      for (int j = 0; j < rows; ++j) tile[j * kPitch + lane] = y[(r0 + j) * ld + f0 + lane];
    }
    __syncthreads();
    if (mine) {
      for (int k = 0; k < frames; ++k) {
        const long t = f0 + k;
        const double y_t = (double)tile[lane * kPitch + k];
        const double x = (Base ? dc_base_data(y_t, b) : y_t) - dc_deconv_mu(la, g, t, T);
        dc_deconv_push(top, n, st, x, t, G, sm);
      }
    }
  }
  if (mine) {
    st.store(n - 1, top);                                            // T >= 1: n >= 1.  The fill kernel reads the workspace only
    pools[r] = n;
  }
}

// The pool of trace r that holds frame t: the last whose start is <= t.  The starts ascend, so a bisection finds it; pool lo starts
// at or before t, pool hi + 1 (if any) after it.  t in the caller's own integer type: the comparison stays as wide as it was there.
template <typename Frame>
__device__ __forceinline__ int32_t pool_of(const int2* tl, long R, long r, int32_t lo, int32_t hi, Frame t) {
  while (lo < hi) {
    const int32_t mid = lo + (hi - lo + 1) / 2;                      // lo < mid <= hi
    if (tl[(long)mid * R + r].x <= t) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// One thread per sample (r, t): pool_of over the trace's n pools.  Every output element is written, each by one product or one
// multiply-subtract.
template <bool Each>
__global__ __launch_bounds__(kFillThreads) void deconv_fill_kernel(const double* __restrict__ ws, const int* __restrict__ pools, int R, long T,
                                                                  double g_all, const double* __restrict__ gs, const double* __restrict__ G_all,
                                                                  long ldG, double* __restrict__ calcium, double* __restrict__ spikes) {
  const long plane = (long)R * T;
  const long idx = (long)blockIdx.x * kFillThreads + threadIdx.x;
  if (idx >= plane) return;
  const long r = idx / T;
  const int32_t t = (int32_t)(idx - r * T);
  const double g = Each ? gs[r] : g_all;
  const double* __restrict__ G = Each ? G_all + r * ldG : G_all;
  const double* v = ws;
  const int2* tl = reinterpret_cast<const int2*>(ws + 2 * plane);
  const int32_t lo = pool_of(tl, R, r, 0, pools[r] - 1, t);
  const int2 own = tl[(long)lo * R + r];
  const int32_t k = t - own.x;
  const double c = dc_deconv_calcium(v[(long)lo * R + r], G[k]);
  double s = 0.0;
  if (k == 0 && lo > 0) {
    const long below = (long)(lo - 1) * R + r;
    s = dc_deconv_spike(c, g, dc_deconv_calcium(v[below], G[tl[below].y - 1]));
  }
  calcium[idx] = c;
  spikes[idx] = s;
}

// ---- the noise-constrained search (csrc/deconv_search_math.h) ---------------------------------------------------------------------
// The state of the searches: five planes of R 8-byte words -- lo, hi, rss_lo, target (doubles), phase (an integer).
struct SearchState {
  double* w;
  long R;
  __device__ __forceinline__ DcSearch load(long r) const {
    DcSearch s;
    s.lo = w[r];
    s.hi = w[R + r];
    s.rss_lo = w[2 * R + r];
    s.target = w[3 * R + r];
    s.phase = (int32_t) reinterpret_cast<const long*>(w + 4 * R)[r];
    return s;
  }
  __device__ __forceinline__ void store(long r, const DcSearch& s) {
    w[r] = s.lo;
    w[R + r] = s.hi;
    w[2 * R + r] = s.rss_lo;
    w[3 * R + r] = s.target;
    reinterpret_cast<long*>(w + 4 * R)[r] = s.phase;
  }
};

// one thread per trace: the state before round 0, and round 0's parameter
__global__ __launch_bounds__(kSearchThreads) void deconv_search_begin_kernel(const double* __restrict__ sigma, int R, long T, double* state,
                                                                             double* __restrict__ param) {
  const long r = (long)blockIdx.x * kSearchThreads + threadIdx.x;
  if (r >= R) return;
  SearchState st = {state, (long)R};
  st.store(r, dc_search_begin(sigma[r], T));
  param[r] = 0.0;
}

// The residual of the stacks the forward pass left in the workspace, then one step of the search.  One workgroup of 256 threads per
// trace: thread j owns lane j of the fold, t = j, j + 256, ... (coalesced reads of y); the pool of t is found as the fill kernel
// finds it (pool_of), from the pool of the thread's previous frame upwards and only when t has left that pool.  The tree through
// LDS is dc_dyn_fold_tree of trace_dyn_math.h; thread 0 then moves the bracket and writes the parameter the next forward
// pass reads (last: p*, RSS(p*) and the status instead).  Every word has one writer; frames t >= T of a row are never read.
template <typename In, bool Each>
__global__ __launch_bounds__(kSearchThreads) void deconv_residual_step_kernel(const In* __restrict__ y, long ld, int R, long T,
                                                                              const double* __restrict__ G_all, long ldG,
                                                                              const double* __restrict__ ws, const int* __restrict__ pools, int last,
                                                                              double* state, double* param, double* __restrict__ rss,
                                                                              int* __restrict__ status) {
  __shared__ double red[kSearchThreads];
  const int tid = threadIdx.x;
  const long plane = (long)R * T;
  const double* v = ws;
  const int2* tl = reinterpret_cast<const int2*>(ws + 2 * plane);
  for (long r = blockIdx.x; r < R; r += gridDim.x) {
    const In* __restrict__ row = y + r * ld;
    const double* __restrict__ G = Each ? G_all + r * ldG : G_all;
    const int32_t n = pools[r];
    int32_t at = 0, start = 0, end = 0;                              // the pool of the previous frame: [start, end); none yet
    double val = 0.0;
    double s = 0.0;
    for (long t = tid; t < T; t += kSearchThreads) {
      if (t >= end) {
        at = pool_of(tl, R, r, at, n - 1, t);
        const int2 own = tl[(long)at * R + r];
        start = own.x;
        end = own.x + own.y;
        val = v[(long)at * R + r];
      }
      s = s + dc_search_term((double)row[t], dc_deconv_calcium(val, G[t - start]));
    }
    red[tid] = s;
    dc_dyn_fold_tree(red, 1);                                        // its last barrier frees red[1 ..] for the next trace
    if (tid == 0) {                                                  // red[0] is thread 0's own: read here, written next after this
      SearchState st = {state, (long)R};
      DcSearch q = st.load(r);
      const double next = dc_search_step(q, param[r], red[0]);
      st.store(r, q);
      if (last) {
        param[r] = q.lo;
        rss[r] = q.rss_lo;
        status[r] = dc_search_status(q);
      } else {
        param[r] = next;
      }
    }
  }
}

template <typename In>
void deconv_host_row(const In* y, long T, double g, const double* G, double lam, double smin, std::vector<DcPool>& pool, double* calcium,
                     double* spikes, int* pools) {
  const int32_t n = dc_deconv_forward_host(y, T, g, G, lam, smin, pool);
  *pools = n;
  for (int32_t i = 0; i < n; ++i) {
    const DcPool& p = pool[(size_t)i];
    for (int32_t k = 0; k < p.l; ++k) {
      calcium[p.t0 + k] = dc_deconv_calcium(p.v, G[k]);
      spikes[p.t0 + k] = 0.0;
    }
    if (i > 0) spikes[p.t0] = dc_deconv_spike(calcium[p.t0], g, calcium[p.t0 - 1]);
  }
}

int check_limits(const char* who, int R, long T, double g) {
  DC_REQUIRE(g > 0.0 && g < 1.0, DC_EINVAL, "%s: g = %g is outside (0, 1)", who, g);      // a NaN fails both comparisons
  return dc_trace_check_limits(who, R, T);
}

// the forward pass; the arguments have been checked
template <bool Each, bool Base>
int launch_forward_as(const char* who, const void* y, int is_f64, long ld, int R, long T, double g, const double* gs, const double* G, long ldG,
                      const double* lam, const double* smin, const double* base, void* ws, int* pools, dc_stream_t stream) {
  const unsigned groups = (unsigned)(((long)R + kLanes - 1) / kLanes);                      // <= 2^25: no cap
  if (is_f64)
    hipLaunchKernelGGL((deconv_forward_kernel<double, Each, Base>), dim3(groups), dim3(kLanes), 0, (hipStream_t)stream, (const double*)y, ld, R, T,
                       g, gs, G, ldG, lam, smin, base, (double*)ws, pools);
  else
    hipLaunchKernelGGL((deconv_forward_kernel<float, Each, Base>), dim3(groups), dim3(kLanes), 0, (hipStream_t)stream, (const float*)y, ld, R, T, g,
                       gs, G, ldG, lam, smin, base, (double*)ws, pools);
  DC_CHECK_LAUNCH(who);
  return DC_OK;
}

// base == nullptr: no baseline, the kernel of the entry points that have none
template <bool Each>
int launch_forward(const char* who, const void* y, int is_f64, long ld, int R, long T, double g, const double* gs, const double* G, long ldG,
                   const double* lam, const double* smin, const double* base, void* ws, int* pools, dc_stream_t stream) {
  if (base) return launch_forward_as<Each, true>(who, y, is_f64, ld, R, T, g, gs, G, ldG, lam, smin, base, ws, pools, stream);
  return launch_forward_as<Each, false>(who, y, is_f64, ld, R, T, g, gs, G, ldG, lam, smin, nullptr, ws, pools, stream);
}

// the forward pass, then the fill; the arguments have been checked
template <bool Each>
int launch_deconv(const char* who, const void* y, int is_f64, long ld, int R, long T, double g, const double* gs, const double* G, long ldG,
                  const double* lam, const double* smin, const double* base, void* ws, double* calcium, double* spikes, int* pools,
                  dc_stream_t stream) {
  const int rc = launch_forward<Each>(who, y, is_f64, ld, R, T, g, gs, G, ldG, lam, smin, base, ws, pools, stream);
  if (rc != DC_OK) return rc;
  const unsigned blocks = (unsigned)(((long)R * T + kFillThreads - 1) / kFillThreads);      // <= 2^23: no cap
  hipLaunchKernelGGL(deconv_fill_kernel<Each>, dim3(blocks), dim3(kFillThreads), 0, (hipStream_t)stream, (const double*)ws, pools, R, T, g, gs, G,
                     ldG, calcium, spikes);
  DC_CHECK_LAUNCH(who);
  return DC_OK;
}

}  // namespace

extern "C" long dc_trace_deconv_ws_bytes(int R, long T) {
  if (R <= 0 || T <= 0 || T > DC_TRACE_DECONV_MAX_FRAMES || (long)R * T > DC_TRACE_DECONV_MAX_SAMPLES) return 0;
  return 24L * R * T;
}

extern "C" int dc_trace_deconv_ar1(const void* y, int is_f64, long ld, int R, long T, double g, const double* G, const double* lam,
                                   const double* smin, void* ws, double* calcium, double* spikes, int* pools, dc_stream_t stream) {
  const char* who = "dc_trace_deconv_ar1";
  DC_REQUIRE(G && lam && smin && ws && calcium && spikes && pools, DC_EINVAL, "%s: null pointer", who);
  int rc = dc_trace_check_counts(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  rc = check_limits(who, R, T, g);
  if (rc != DC_OK) return rc;
  DC_REQUIRE(dc_aligned(7, G, lam, smin, ws, calcium, spikes) && dc_aligned(3, pools) && dc_trace_aligned(y, is_f64), DC_EINVAL, "%s: misaligned buffer", who);
  if (R == 0 || T == 0) return DC_OK;
  return launch_deconv<false>(who, y, is_f64, ld, R, T, g, nullptr, G, 0, lam, smin, nullptr, ws, calcium, spikes, pools, stream);
}

extern "C" int dc_trace_deconv_ar1_each(const void* y, int is_f64, long ld, int R, long T, const double* g, const double* G, long ldG,
                                        const double* lam, const double* smin, void* ws, double* calcium, double* spikes, int* pools,
                                        dc_stream_t stream) {
  const char* who = "dc_trace_deconv_ar1_each";
  DC_REQUIRE(g && G && lam && smin && ws && calcium && spikes && pools, DC_EINVAL, "%s: null pointer", who);
  int rc = dc_trace_check_counts(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  DC_REQUIRE(ldG >= T + 1, DC_EINVAL, "%s: ldG = %ld is below T + 1 = %ld", who, ldG, T + 1);
  rc = check_limits(who, R, T, 0.5);                                 // the decays lie in device memory: THE CALLER PROMISES 0 < g[r] < 1
  if (rc != DC_OK) return rc;
  DC_REQUIRE(dc_aligned(7, g, G, lam, smin, ws, calcium, spikes) && dc_aligned(3, pools) && dc_trace_aligned(y, is_f64), DC_EINVAL, "%s: misaligned buffer", who);
  if (R == 0 || T == 0) return DC_OK;
  return launch_deconv<true>(who, y, is_f64, ld, R, T, 0.0, g, G, ldG, lam, smin, nullptr, ws, calcium, spikes, pools, stream);
}

extern "C" int dc_trace_deconv_ar1_host(const void* y, int is_f64, long ld, int R, long T, const double* G, const double* lam,
                                        const double* smin, double* calcium, double* spikes, int* pools) {
  const char* who = "dc_trace_deconv_ar1_host";
  DC_REQUIRE(G && lam && smin && calcium && spikes && pools, DC_EINVAL, "%s: null pointer", who);
  DC_REQUIRE(dc_aligned(7, G, lam, smin, calcium, spikes) && dc_aligned(3, pools) && dc_trace_aligned(y, is_f64), DC_EINVAL, "%s: misaligned buffer", who);
  int rc = dc_trace_check_counts(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  if (R == 0 || T == 0) return DC_OK;                                // G is not read: without frames it need not hold g
  DC_REQUIRE(G[0] == 1.0, DC_EINVAL, "%s: G[0] = %g is not 1", who, G[0]);
  const double g = G[1];
  rc = check_limits(who, R, T, g);
  if (rc != DC_OK) return rc;
  for (int r = 0; r < R; ++r)
    DC_REQUIRE(lam[r] >= 0.0 && smin[r] >= 0.0, DC_EINVAL, "%s: trace %d: lam = %g, smin = %g: neither may be negative", who, r, lam[r], smin[r]);
  std::vector<DcPool> pool((size_t)T);
  for (int r = 0; r < R; ++r) {
    double* c = calcium + (long)r * T;
    double* s = spikes + (long)r * T;
    if (is_f64)
      deconv_host_row((const double*)y + (long)r * ld, T, g, G, lam[r], smin[r], pool, c, s, pools + r);
    else
      deconv_host_row((const float*)y + (long)r * ld, T, g, G, lam[r], smin[r], pool, c, s, pools + r);
  }
  return DC_OK;
}

// ---- the noise-constrained search --------------------------------------------------------------------------------------------------
namespace {

// the residual of the stacks in ws and one step of every search; the arguments have been checked
template <bool Each>
int launch_residual_step(const char* who, const void* y, int is_f64, long ld, int R, long T, const double* G, long ldG, const void* ws,
                         const int* pools, int last, void* state, double* param, double* rss, int* status, dc_stream_t stream) {
  const unsigned groups = (unsigned)(R < kSearchMaxGroups ? R : kSearchMaxGroups);
  if (is_f64)
    hipLaunchKernelGGL((deconv_residual_step_kernel<double, Each>), dim3(groups), dim3(kSearchThreads), 0, (hipStream_t)stream, (const double*)y, ld,
                       R, T, G, ldG, (const double*)ws, pools, last, (double*)state, param, rss, status);
  else
    hipLaunchKernelGGL((deconv_residual_step_kernel<float, Each>), dim3(groups), dim3(kSearchThreads), 0, (hipStream_t)stream, (const float*)y, ld, R,
                       T, G, ldG, (const double*)ws, pools, last, (double*)state, param, rss, status);
  DC_CHECK_LAUNCH(who);
  return DC_OK;
}

// round 0, the rounds and the final pass; the arguments have been checked
template <bool Each>
int launch_constrained(const char* who, const void* y, int is_f64, long ld, int R, long T, double g, const double* gs, const double* G, long ldG,
                       int which, const double* sigma, const double* other, int rounds, void* ws, void* state, double* calcium, double* spikes,
                       int* pools, double* param, double* rss, int* status, dc_stream_t stream) {
  const double* lam = which == DC_SEARCH_LAM ? param : other;
  const double* smin = which == DC_SEARCH_LAM ? other : param;
  const unsigned begin = (unsigned)(((long)R + kSearchThreads - 1) / kSearchThreads);
  hipLaunchKernelGGL(deconv_search_begin_kernel, dim3(begin), dim3(kSearchThreads), 0, (hipStream_t)stream, sigma, R, T, (double*)state, param);
  DC_CHECK_LAUNCH(who);
  for (int round = 0; round <= rounds; ++round) {
    int rc = launch_forward<Each>(who, y, is_f64, ld, R, T, g, gs, G, ldG, lam, smin, nullptr, ws, pools, stream);
    if (rc != DC_OK) return rc;
    rc = launch_residual_step<Each>(who, y, is_f64, ld, R, T, G, ldG, ws, pools, round == rounds, state, param, rss, status, stream);
    if (rc != DC_OK) return rc;
  }
  return launch_deconv<Each>(who, y, is_f64, ld, R, T, g, gs, G, ldG, lam, smin, nullptr, ws, calcium, spikes, pools, stream);
}

int check_search(const char* who, int which, int rounds) {
  DC_REQUIRE(which == DC_SEARCH_SMIN || which == DC_SEARCH_LAM, DC_EINVAL, "%s: which = %d is neither 0 (smin) nor 1 (lam)", who, which);
  DC_REQUIRE(rounds >= 1 && rounds <= DC_SEARCH_MAX_ROUNDS, DC_EINVAL, "%s: rounds = %d is outside [1, %d]", who, rounds, DC_SEARCH_MAX_ROUNDS);
  return DC_OK;
}

}  // namespace

extern "C" long dc_trace_deconv_search_state_bytes(int R) { return R <= 0 ? 0 : 40L * R; }

extern "C" int dc_trace_deconv_ar1_constrained(const void* y, int is_f64, long ld, int R, long T, double g, const double* gs, const double* G,
                                               long ldG, int which, const double* sigma, const double* fixed_other, int rounds, void* ws,
                                               void* state, double* calcium, double* spikes, int* pools, double* param, double* rss,
                                               int* status, dc_stream_t stream) {
  const char* who = "dc_trace_deconv_ar1_constrained";
  DC_REQUIRE(G && sigma && fixed_other && ws && state && calcium && spikes && pools && param && rss && status, DC_EINVAL, "%s: null pointer", who);
  int rc = dc_trace_check_counts(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  rc = check_search(who, which, rounds);
  if (rc != DC_OK) return rc;
  if (gs) DC_REQUIRE(ldG >= T + 1, DC_EINVAL, "%s: ldG = %ld is below T + 1 = %ld", who, ldG, T + 1);
  rc = check_limits(who, R, T, gs ? 0.5 : g);                        // per trace, the decays lie in device memory: THE CALLER PROMISES 0 < gs[r] < 1
  if (rc != DC_OK) return rc;                                        // sigma, fixed_other likewise: THE CALLER PROMISES 0 <= sigma[r] < 2^500, finite, and fixed_other[r] >= 0
  DC_REQUIRE(dc_aligned(7, gs, G, sigma, fixed_other, ws, state, calcium, spikes, param, rss) && dc_aligned(3, pools, status) &&
                 dc_trace_aligned(y, is_f64),
             DC_EINVAL, "%s: misaligned buffer", who);
  if (R == 0 || T == 0) return DC_OK;
  if (gs)
    return launch_constrained<true>(who, y, is_f64, ld, R, T, 0.0, gs, G, ldG, which, sigma, fixed_other, rounds, ws, state, calcium, spikes, pools,
                                    param, rss, status, stream);
  return launch_constrained<false>(who, y, is_f64, ld, R, T, g, nullptr, G, 0, which, sigma, fixed_other, rounds, ws, state, calcium, spikes, pools,
                                   param, rss, status, stream);
}

extern "C" int dc_trace_deconv_search_step(const void* y, int is_f64, long ld, int R, long T, const double* G, long ldG, const void* ws,
                                           const int* pools, int last, void* state, double* param, double* rss, int* status,
                                           dc_stream_t stream) {
  const char* who = "dc_trace_deconv_search_step";
  DC_REQUIRE(G && ws && pools && state && param && rss && status, DC_EINVAL, "%s: null pointer", who);
  int rc = dc_trace_check_counts(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  DC_REQUIRE(last == 0 || last == 1, DC_EINVAL, "%s: last = %d is neither 0 nor 1", who, last);
  DC_REQUIRE(ldG == 0 || ldG >= T + 1, DC_EINVAL, "%s: ldG = %ld is neither 0 nor at least T + 1 = %ld", who, ldG, T + 1);
  rc = check_limits(who, R, T, 0.5);
  if (rc != DC_OK) return rc;
  DC_REQUIRE(dc_aligned(7, G, ws, state, param, rss) && dc_aligned(3, pools, status) && dc_trace_aligned(y, is_f64), DC_EINVAL, "%s: misaligned buffer", who);
  if (R == 0 || T == 0) return DC_OK;
  if (ldG) return launch_residual_step<true>(who, y, is_f64, ld, R, T, G, ldG, ws, pools, last, state, param, rss, status, stream);
  return launch_residual_step<false>(who, y, is_f64, ld, R, T, G, 0, ws, pools, last, state, param, rss, status, stream);
}

extern "C" int dc_trace_deconv_ar1_constrained_host(const void* y, int is_f64, long ld, int R, long T, const double* G, int which,
                                                    const double* sigma, const double* fixed_other, int rounds, double* calcium, double* spikes,
                                                    int* pools, double* param, double* rss, int* status) {
  const char* who = "dc_trace_deconv_ar1_constrained_host";
  DC_REQUIRE(G && sigma && fixed_other && calcium && spikes && pools && param && rss && status, DC_EINVAL, "%s: null pointer", who);
  DC_REQUIRE(dc_aligned(7, G, sigma, fixed_other, calcium, spikes, param, rss) && dc_aligned(3, pools, status) && dc_trace_aligned(y, is_f64),
             DC_EINVAL, "%s: misaligned buffer", who);
  int rc = dc_trace_check_counts(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  rc = check_search(who, which, rounds);
  if (rc != DC_OK) return rc;
  if (R == 0 || T == 0) return DC_OK;                                // G is not read: without frames it need not hold g
  DC_REQUIRE(G[0] == 1.0, DC_EINVAL, "%s: G[0] = %g is not 1", who, G[0]);
  const double g = G[1];
  rc = check_limits(who, R, T, g);
  if (rc != DC_OK) return rc;
  for (int r = 0; r < R; ++r) {
    DC_REQUIRE(sigma[r] >= 0.0 && sigma[r] < 0x1p500, DC_EINVAL, "%s: trace %d: sigma = %g is outside [0, 2^500)", who, r, sigma[r]);
    DC_REQUIRE(fixed_other[r] >= 0.0, DC_EINVAL, "%s: trace %d: the fixed parameter %g is negative", who, r, fixed_other[r]);
  }
  std::vector<DcPool> pool((size_t)T);
  std::vector<double> scratch((size_t)T);
  for (int r = 0; r < R; ++r) {
    double* c = calcium + (long)r * T;
    double* s = spikes + (long)r * T;
    if (is_f64) {
      const double* row = (const double*)y + (long)r * ld;
      dc_search_host(row, T, g, G, which, sigma[r], fixed_other[r], rounds, pool, scratch.data(), param + r, rss + r, status + r);
      deconv_host_row(row, T, g, G, which == DC_SEARCH_LAM ? param[r] : fixed_other[r], which == DC_SEARCH_LAM ? fixed_other[r] : param[r], pool, c, s,
                      pools + r);
    } else {
      const float* row = (const float*)y + (long)r * ld;
      dc_search_host(row, T, g, G, which, sigma[r], fixed_other[r], rounds, pool, scratch.data(), param + r, rss + r, status + r);
      deconv_host_row(row, T, g, G, which == DC_SEARCH_LAM ? param[r] : fixed_other[r], which == DC_SEARCH_LAM ? fixed_other[r] : param[r], pool, c, s,
                      pools + r);
    }
  }
  return DC_OK;
}

// ---- a baseline in the deconvolution (csrc/deconv_base_math.h) -----------------------------------------------------------------------
namespace {

// The state of the joint searches: seven planes of R 8-byte words -- the five of SearchState, then b (carried) and b_lo.
struct BaseSearchState {
  double* w;
  long R;
  __device__ __forceinline__ DcBaseSearch load(long r) const {
    SearchState st = {w, R};
    DcBaseSearch q;
    q.s = st.load(r);
    q.b = w[5 * R + r];
    q.b_lo = w[6 * R + r];
    return q;
  }
  __device__ __forceinline__ void store(long r, const DcBaseSearch& q) {
    SearchState st = {w, R};
    st.store(r, q.s);
    w[5 * R + r] = q.b;
    w[6 * R + r] = q.b_lo;
  }
};

// one thread per trace: the state before round 0 (base holds b_0 and stays), and round 0's parameter
__global__ __launch_bounds__(kSearchThreads) void deconv_base_begin_kernel(const double* __restrict__ sigma, const double* __restrict__ base, int R,
                                                                           long T, double* state, double* __restrict__ param) {
  const long r = (long)blockIdx.x * kSearchThreads + threadIdx.x;
  if (r >= R) return;
  BaseSearchState st = {state, (long)R};
  st.store(r, dc_base_search_begin(sigma[r], T, base[r]));
  param[r] = 0.0;
}

// The three folds of the stacks the forward pass left in the workspace at the baseline base[r] -- RSS, S and A of
// deconv_base_math.h, in one sweep shaped like deconv_residual_step_kernel's: thread j owns lane j of each fold, t = j, j + 256, ...;
// the pool of t is looked up (pool_of) only when t has left the pool of the thread's previous frame.  The tree runs over the three
// folds at once (dc_dyn_fold_tree, rows = 3); its results red[0], red[256] and red[512] are thread 0's own words.  Thread 0 then does
// what `mode` says: the baseline step (DC_BASE_FIT; DC_BASE_PASS_A, which also keeps it in the state) or the step of the search
// (DC_BASE_PASS_B; DC_BASE_PASS_LAST writes p*, b*, the residual and the status).  sums, where given, takes the three folds as planes
// of R doubles.  Every word has one writer; frames t >= T of a row are never read.
template <typename In, bool Each>
__global__ __launch_bounds__(kSearchThreads) void deconv_base_step_kernel(const In* __restrict__ y, long ld, int R, long T,
                                                                          const double* __restrict__ G_all, long ldG,
                                                                          const double* __restrict__ ws, const int* __restrict__ pools, int mode,
                                                                          double* state, double* param, double* base, double* __restrict__ rss,
                                                                          int* __restrict__ status, double* __restrict__ sums) {
  __shared__ double red[3 * kSearchThreads];
  const int tid = threadIdx.x;
  const long plane = (long)R * T;
  const double* v = ws;
  const int2* tl = reinterpret_cast<const int2*>(ws + 2 * plane);
  for (long r = blockIdx.x; r < R; r += gridDim.x) {
    const In* __restrict__ row = y + r * ld;
    const double* __restrict__ G = Each ? G_all + r * ldG : G_all;
    const double g = G[1];                                           // T >= 1: the table has the entry
    const double b = base[r];                                        // thread 0 writes it after the tree: its barriers lie between
    const int32_t n = pools[r];
    int32_t at = 0, start = 0, end = 0;                              // the pool of the previous frame: [start, end); none yet
    double val = 0.0, Gl = 1.0;
    double q = 0.0, s = 0.0, a = 0.0;
    for (long t = tid; t < T; t += kSearchThreads) {
      if (t >= end) {
        at = pool_of(tl, R, r, at, n - 1, t);
        const int2 own = tl[(long)at * R + r];
        start = own.x;
        end = own.x + own.y;
        val = v[(long)at * R + r];
        Gl = G[own.y];
      }
      const double d = dc_base_resid((double)row[t], b, dc_deconv_calcium(val, G[t - start]));
      q = q + d * d;
      s = s + d;
      a = a + dc_base_gain_at(val, t, start, g, Gl);
    }
    red[tid] = q;
    red[kSearchThreads + tid] = s;
    red[2 * kSearchThreads + tid] = a;
    dc_dyn_fold_tree(red, 3);                                        // its last barrier frees all but thread 0's words for the next trace
    if (tid == 0) {
      const double RSS = red[0], S = red[kSearchThreads], A = red[2 * kSearchThreads];
      if (sums) {
        sums[r] = RSS;
        sums[(long)R + r] = S;
        sums[2L * R + r] = A;
      }
      if (mode == DC_BASE_FIT) {
        base[r] = dc_base_step(b, S, A, T);
      } else {
        BaseSearchState st = {state, (long)R};
        DcBaseSearch x = st.load(r);
        if (mode == DC_BASE_PASS_A) {
          base[r] = dc_base_search_newton(x, S, A, T);
          st.store(r, x);
        } else {
          const double next = dc_base_search_step(x, param[r], RSS);
          st.store(r, x);
          if (mode == DC_BASE_PASS_LAST) {
            param[r] = x.s.lo;
            base[r] = x.b_lo;
            rss[r] = x.s.rss_lo;
            status[r] = dc_search_status(x.s);
          } else {
            param[r] = next;
          }
        }
      }
    }
  }
}

// the three folds of the stacks in ws and what `mode` does with them; the arguments have been checked
template <bool Each>
int launch_base_step(const char* who, const void* y, int is_f64, long ld, int R, long T, const double* G, long ldG, const void* ws,
                     const int* pools, int mode, void* state, double* param, double* base, double* rss, int* status, double* sums,
                     dc_stream_t stream) {
  const unsigned groups = (unsigned)(R < kSearchMaxGroups ? R : kSearchMaxGroups);
  if (is_f64)
    hipLaunchKernelGGL((deconv_base_step_kernel<double, Each>), dim3(groups), dim3(kSearchThreads), 0, (hipStream_t)stream, (const double*)y, ld, R,
                       T, G, ldG, (const double*)ws, pools, mode, (double*)state, param, base, rss, status, sums);
  else
    hipLaunchKernelGGL((deconv_base_step_kernel<float, Each>), dim3(groups), dim3(kSearchThreads), 0, (hipStream_t)stream, (const float*)y, ld, R, T,
                       G, ldG, (const double*)ws, pools, mode, (double*)state, param, base, rss, status, sums);
  DC_CHECK_LAUNCH(who);
  return DC_OK;
}

// `rounds` baseline steps, then the forward pass and the fill at b_N; the arguments have been checked
template <bool Each>
int launch_fit_base(const char* who, const void* y, int is_f64, long ld, int R, long T, double g, const double* gs, const double* G, long ldG,
                    const double* lam, const double* smin, int rounds, void* ws, double* calcium, double* spikes, int* pools, double* base,
                    dc_stream_t stream) {
  for (int round = 0; round < rounds; ++round) {
    int rc = launch_forward<Each>(who, y, is_f64, ld, R, T, g, gs, G, ldG, lam, smin, base, ws, pools, stream);
    if (rc != DC_OK) return rc;
    rc = launch_base_step<Each>(who, y, is_f64, ld, R, T, G, ldG, ws, pools, DC_BASE_FIT, nullptr, nullptr, base, nullptr, nullptr, nullptr, stream);
    if (rc != DC_OK) return rc;
  }
  return launch_deconv<Each>(who, y, is_f64, ld, R, T, g, gs, G, ldG, lam, smin, base, ws, calcium, spikes, pools, stream);
}

// round 0, the rounds of two passes each and the final pass; the arguments have been checked
template <bool Each>
int launch_constrained_base(const char* who, const void* y, int is_f64, long ld, int R, long T, double g, const double* gs, const double* G,
                            long ldG, int which, const double* sigma, const double* other, int rounds, void* ws, void* state, double* calcium,
                            double* spikes, int* pools, double* param, double* base, double* rss, int* status, dc_stream_t stream) {
  const double* lam = which == DC_SEARCH_LAM ? param : other;
  const double* smin = which == DC_SEARCH_LAM ? other : param;
  const unsigned begin = (unsigned)(((long)R + kSearchThreads - 1) / kSearchThreads);
  hipLaunchKernelGGL(deconv_base_begin_kernel, dim3(begin), dim3(kSearchThreads), 0, (hipStream_t)stream, sigma, (const double*)base, R, T,
                     (double*)state, param);
  DC_CHECK_LAUNCH(who);
  for (int round = 0; round <= rounds; ++round) {
    int rc;
    if (round > 0) {                                                 // pass A: the baseline step at (p, b)
      rc = launch_forward<Each>(who, y, is_f64, ld, R, T, g, gs, G, ldG, lam, smin, base, ws, pools, stream);
      if (rc != DC_OK) return rc;
      rc = launch_base_step<Each>(who, y, is_f64, ld, R, T, G, ldG, ws, pools, DC_BASE_PASS_A, state, param, base, rss, status, nullptr, stream);
      if (rc != DC_OK) return rc;
    }
    rc = launch_forward<Each>(who, y, is_f64, ld, R, T, g, gs, G, ldG, lam, smin, base, ws, pools, stream);      // pass B: RSS at (p, b')
    if (rc != DC_OK) return rc;
    rc = launch_base_step<Each>(who, y, is_f64, ld, R, T, G, ldG, ws, pools, round == rounds ? DC_BASE_PASS_LAST : DC_BASE_PASS_B, state, param, base,
                                rss, status, nullptr, stream);
    if (rc != DC_OK) return rc;
  }
  return launch_deconv<Each>(who, y, is_f64, ld, R, T, g, gs, G, ldG, lam, smin, base, ws, calcium, spikes, pools, stream);
}

// what the device entry points with a decay per trace or one for all share
int check_decay(const char* who, int R, long T, double g, const double* gs, long ldG) {
  if (gs) DC_REQUIRE(ldG >= T + 1, DC_EINVAL, "%s: ldG = %ld is below T + 1 = %ld", who, ldG, T + 1);
  return check_limits(who, R, T, gs ? 0.5 : g);                      // per trace, the decays lie in device memory: THE CALLER PROMISES 0 < gs[r] < 1
}

// the decay and the table of trace r on the host: one table for all (ldG == 0) or row r; -> DC_OK where the row holds a decay
int host_table(const char* who, const double* G, long ldG, int r, long T, const double** row, double* g) {
  *row = G + (long)r * ldG;
  DC_REQUIRE((*row)[0] == 1.0, DC_EINVAL, "%s: trace %d: G[0] = %g is not 1", who, r, (*row)[0]);
  *g = (*row)[1];
  DC_REQUIRE(*g > 0.0 && *g < 1.0, DC_EINVAL, "%s: trace %d: g = %g is outside (0, 1)", who, r, *g);
  return DC_OK;
}

template <typename In>
void base_host_row(const In* y, long T, double g, const double* G, double lam, double smin, double b, std::vector<DcPool>& pool, double* calcium,
                   double* spikes, int* pools) {
  const int32_t n = dc_base_forward_host(y, T, g, G, lam, smin, b, pool);
  *pools = n;
  for (int32_t i = 0; i < n; ++i) {
    const DcPool& p = pool[(size_t)i];
    for (int32_t k = 0; k < p.l; ++k) {
      calcium[p.t0 + k] = dc_deconv_calcium(p.v, G[k]);
      spikes[p.t0 + k] = 0.0;
    }
    if (i > 0) spikes[p.t0] = dc_deconv_spike(calcium[p.t0], g, calcium[p.t0 - 1]);
  }
}

}  // namespace

extern "C" long dc_trace_deconv_base_state_bytes(int R) { return R <= 0 ? 0 : 56L * R; }

extern "C" int dc_trace_deconv_ar1_base(const void* y, int is_f64, long ld, int R, long T, double g, const double* gs, const double* G, long ldG,
                                        const double* lam, const double* smin, const double* base, void* ws, double* calcium, double* spikes,
                                        int* pools, dc_stream_t stream) {
  const char* who = "dc_trace_deconv_ar1_base";
  DC_REQUIRE(G && lam && smin && base && ws && calcium && spikes && pools, DC_EINVAL, "%s: null pointer", who);
  int rc = dc_trace_check_counts(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  rc = check_decay(who, R, T, g, gs, ldG);
  if (rc != DC_OK) return rc;                                        // base likewise: THE CALLER PROMISES FINITE VALUES
  DC_REQUIRE(dc_aligned(7, gs, G, lam, smin, base, ws, calcium, spikes) && dc_aligned(3, pools) && dc_trace_aligned(y, is_f64), DC_EINVAL,
             "%s: misaligned buffer", who);
  if (R == 0 || T == 0) return DC_OK;
  if (gs) return launch_deconv<true>(who, y, is_f64, ld, R, T, 0.0, gs, G, ldG, lam, smin, base, ws, calcium, spikes, pools, stream);
  return launch_deconv<false>(who, y, is_f64, ld, R, T, g, nullptr, G, 0, lam, smin, base, ws, calcium, spikes, pools, stream);
}

extern "C" int dc_trace_deconv_ar1_fit_base(const void* y, int is_f64, long ld, int R, long T, double g, const double* gs, const double* G,
                                            long ldG, const double* lam, const double* smin, int rounds, void* ws, double* calcium,
                                            double* spikes, int* pools, double* base, dc_stream_t stream) {
  const char* who = "dc_trace_deconv_ar1_fit_base";
  DC_REQUIRE(G && lam && smin && ws && calcium && spikes && pools && base, DC_EINVAL, "%s: null pointer", who);
  int rc = dc_trace_check_counts(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  DC_REQUIRE(rounds >= 1 && rounds <= DC_BASE_MAX_ROUNDS, DC_EINVAL, "%s: rounds = %d is outside [1, %d]", who, rounds, DC_BASE_MAX_ROUNDS);
  rc = check_decay(who, R, T, g, gs, ldG);
  if (rc != DC_OK) return rc;
  DC_REQUIRE(dc_aligned(7, gs, G, lam, smin, ws, calcium, spikes, base) && dc_aligned(3, pools) && dc_trace_aligned(y, is_f64), DC_EINVAL,
             "%s: misaligned buffer", who);
  if (R == 0 || T == 0) return DC_OK;
  if (gs) return launch_fit_base<true>(who, y, is_f64, ld, R, T, 0.0, gs, G, ldG, lam, smin, rounds, ws, calcium, spikes, pools, base, stream);
  return launch_fit_base<false>(who, y, is_f64, ld, R, T, g, nullptr, G, 0, lam, smin, rounds, ws, calcium, spikes, pools, base, stream);
}

extern "C" int dc_trace_deconv_ar1_constrained_base(const void* y, int is_f64, long ld, int R, long T, double g, const double* gs, const double* G,
                                                    long ldG, int which, const double* sigma, const double* fixed_other, int rounds, void* ws,
                                                    void* state, double* calcium, double* spikes, int* pools, double* param, double* base,
                                                    double* rss, int* status, dc_stream_t stream) {
  const char* who = "dc_trace_deconv_ar1_constrained_base";
  DC_REQUIRE(G && sigma && fixed_other && ws && state && calcium && spikes && pools && param && base && rss && status, DC_EINVAL,
             "%s: null pointer", who);
  int rc = dc_trace_check_counts(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  rc = check_search(who, which, rounds);
  if (rc != DC_OK) return rc;
  rc = check_decay(who, R, T, g, gs, ldG);
  if (rc != DC_OK) return rc;                                        // sigma, fixed_other, base: THE CALLER PROMISES the ranges of the header
  DC_REQUIRE(dc_aligned(7, gs, G, sigma, fixed_other, ws, state, calcium, spikes, param, base, rss) && dc_aligned(3, pools, status) &&
                 dc_trace_aligned(y, is_f64),
             DC_EINVAL, "%s: misaligned buffer", who);
  if (R == 0 || T == 0) return DC_OK;
  if (gs)
    return launch_constrained_base<true>(who, y, is_f64, ld, R, T, 0.0, gs, G, ldG, which, sigma, fixed_other, rounds, ws, state, calcium, spikes,
                                         pools, param, base, rss, status, stream);
  return launch_constrained_base<false>(who, y, is_f64, ld, R, T, g, nullptr, G, 0, which, sigma, fixed_other, rounds, ws, state, calcium, spikes,
                                        pools, param, base, rss, status, stream);
}

extern "C" int dc_trace_deconv_base_step(const void* y, int is_f64, long ld, int R, long T, const double* G, long ldG, const void* ws,
                                         const int* pools, int mode, void* state, double* param, double* base, double* rss, int* status,
                                         double* sums, dc_stream_t stream) {
  const char* who = "dc_trace_deconv_base_step";
  DC_REQUIRE(mode >= DC_BASE_FIT && mode <= DC_BASE_PASS_LAST, DC_EINVAL, "%s: mode = %d is outside [0, 3]", who, mode);
  DC_REQUIRE(G && ws && pools && base, DC_EINVAL, "%s: null pointer", who);
  if (mode != DC_BASE_FIT) DC_REQUIRE(state && param && rss && status, DC_EINVAL, "%s: null pointer", who);
  int rc = dc_trace_check_counts(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  DC_REQUIRE(ldG == 0 || ldG >= T + 1, DC_EINVAL, "%s: ldG = %ld is neither 0 nor at least T + 1 = %ld", who, ldG, T + 1);
  rc = check_limits(who, R, T, 0.5);
  if (rc != DC_OK) return rc;
  DC_REQUIRE(dc_aligned(7, G, ws, state, param, base, rss, sums) && dc_aligned(3, pools, status) && dc_trace_aligned(y, is_f64), DC_EINVAL,
             "%s: misaligned buffer", who);
  if (R == 0 || T == 0) return DC_OK;
  if (ldG) return launch_base_step<true>(who, y, is_f64, ld, R, T, G, ldG, ws, pools, mode, state, param, base, rss, status, sums, stream);
  return launch_base_step<false>(who, y, is_f64, ld, R, T, G, 0, ws, pools, mode, state, param, base, rss, status, sums, stream);
}

extern "C" int dc_trace_deconv_ar1_fit_base_host(const void* y, int is_f64, long ld, int R, long T, const double* G, long ldG, const double* lam,
                                                 const double* smin, int rounds, double* calcium, double* spikes, int* pools, double* base) {
  const char* who = "dc_trace_deconv_ar1_fit_base_host";
  DC_REQUIRE(G && lam && smin && calcium && spikes && pools && base, DC_EINVAL, "%s: null pointer", who);
  DC_REQUIRE(dc_aligned(7, G, lam, smin, calcium, spikes, base) && dc_aligned(3, pools) && dc_trace_aligned(y, is_f64), DC_EINVAL,
             "%s: misaligned buffer", who);
  int rc = dc_trace_check_counts(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  DC_REQUIRE(rounds >= 0 && rounds <= DC_BASE_MAX_ROUNDS, DC_EINVAL, "%s: rounds = %d is outside [0, %d]", who, rounds, DC_BASE_MAX_ROUNDS);
  DC_REQUIRE(ldG == 0 || ldG >= T + 1, DC_EINVAL, "%s: ldG = %ld is neither 0 nor at least T + 1 = %ld", who, ldG, T + 1);
  if (R == 0 || T == 0) return DC_OK;                                // G is not read: without frames it need not hold g
  rc = dc_trace_check_limits(who, R, T);
  if (rc != DC_OK) return rc;
  for (int r = 0; r < R; ++r) {
    DC_REQUIRE(lam[r] >= 0.0 && smin[r] >= 0.0, DC_EINVAL, "%s: trace %d: lam = %g, smin = %g: neither may be negative", who, r, lam[r], smin[r]);
    DC_REQUIRE(base[r] - base[r] == 0.0, DC_EINVAL, "%s: trace %d: the baseline %g is not finite", who, r, base[r]);
  }
  std::vector<DcPool> pool((size_t)T);
  std::vector<double> scratch(2 * (size_t)T);
  for (int r = 0; r < R; ++r) {
    const double* row_G;
    double g;
    rc = host_table(who, G, ldG, r, T, &row_G, &g);
    if (rc != DC_OK) return rc;
    double* c = calcium + (long)r * T;
    double* s = spikes + (long)r * T;
    if (is_f64) {
      const double* row = (const double*)y + (long)r * ld;
      base[r] = dc_base_fit_host(row, T, g, row_G, lam[r], smin[r], base[r], rounds, pool, scratch.data(), scratch.data() + T);
      base_host_row(row, T, g, row_G, lam[r], smin[r], base[r], pool, c, s, pools + r);
    } else {
      const float* row = (const float*)y + (long)r * ld;
      base[r] = dc_base_fit_host(row, T, g, row_G, lam[r], smin[r], base[r], rounds, pool, scratch.data(), scratch.data() + T);
      base_host_row(row, T, g, row_G, lam[r], smin[r], base[r], pool, c, s, pools + r);
    }
  }
  return DC_OK;
}

extern "C" int dc_trace_deconv_ar1_constrained_base_host(const void* y, int is_f64, long ld, int R, long T, const double* G, long ldG, int which,
                                                         const double* sigma, const double* fixed_other, int rounds, double* calcium,
                                                         double* spikes, int* pools, double* param, double* base, double* rss, int* status) {
  const char* who = "dc_trace_deconv_ar1_constrained_base_host";
  DC_REQUIRE(G && sigma && fixed_other && calcium && spikes && pools && param && base && rss && status, DC_EINVAL, "%s: null pointer", who);
  DC_REQUIRE(dc_aligned(7, G, sigma, fixed_other, calcium, spikes, param, base, rss) && dc_aligned(3, pools, status) && dc_trace_aligned(y, is_f64),
             DC_EINVAL, "%s: misaligned buffer", who);
  int rc = dc_trace_check_counts(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  rc = check_search(who, which, rounds);
  if (rc != DC_OK) return rc;
  DC_REQUIRE(ldG == 0 || ldG >= T + 1, DC_EINVAL, "%s: ldG = %ld is neither 0 nor at least T + 1 = %ld", who, ldG, T + 1);
  if (R == 0 || T == 0) return DC_OK;                                // G is not read: without frames it need not hold g
  rc = dc_trace_check_limits(who, R, T);
  if (rc != DC_OK) return rc;
  for (int r = 0; r < R; ++r) {
    DC_REQUIRE(sigma[r] >= 0.0 && sigma[r] < 0x1p500, DC_EINVAL, "%s: trace %d: sigma = %g is outside [0, 2^500)", who, r, sigma[r]);
    DC_REQUIRE(fixed_other[r] >= 0.0, DC_EINVAL, "%s: trace %d: the fixed parameter %g is negative", who, r, fixed_other[r]);
    DC_REQUIRE(base[r] - base[r] == 0.0, DC_EINVAL, "%s: trace %d: the baseline %g is not finite", who, r, base[r]);
  }
  std::vector<DcPool> pool((size_t)T);
  std::vector<double> scratch(2 * (size_t)T);
  for (int r = 0; r < R; ++r) {
    const double* row_G;
    double g;
    rc = host_table(who, G, ldG, r, T, &row_G, &g);
    if (rc != DC_OK) return rc;
    double* c = calcium + (long)r * T;
    double* s = spikes + (long)r * T;
    const double b0 = base[r];
    if (is_f64) {
      const double* row = (const double*)y + (long)r * ld;
      dc_base_search_host(row, T, g, row_G, which, sigma[r], fixed_other[r], b0, rounds, pool, scratch.data(), scratch.data() + T, param + r, base + r,
                          rss + r, status + r);
      base_host_row(row, T, g, row_G, which == DC_SEARCH_LAM ? param[r] : fixed_other[r], which == DC_SEARCH_LAM ? fixed_other[r] : param[r], base[r],
                    pool, c, s, pools + r);
    } else {
      const float* row = (const float*)y + (long)r * ld;
      dc_base_search_host(row, T, g, row_G, which, sigma[r], fixed_other[r], b0, rounds, pool, scratch.data(), scratch.data() + T, param + r, base + r,
                          rss + r, status + r);
      base_host_row(row, T, g, row_G, which == DC_SEARCH_LAM ? param[r] : fixed_other[r], which == DC_SEARCH_LAM ? fixed_other[r] : param[r], base[r],
                    pool, c, s, pools + r);
    }
  }
  return DC_OK;
}
