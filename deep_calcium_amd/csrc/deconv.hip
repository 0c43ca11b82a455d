// Spikes by deconvolution on the device (include/dcunet.h, "Spikes by deconvolution"): float (R,T) traces, dF/F as dc_trace_baseline
// leaves them -> the non-negative AR(1) calcium c and the spikes s = c[t] - g c[t-1] that fit them best, by the pool-merging
// (OASIS-style) forward pass of csrc/deconv_math.h.  The reference has no counterpart; the header's definitions are the
// specification.  A trace is a strictly sequential computation, so the forward kernel gives one LANE to a trace and the memory
// layout is the work: the traces are row-major, so a wave's lanes would read at stride ld; a tile of 64 traces x 64 frames is
// staged through LDS with coalesced row reads instead and every lane then walks its own row of the tile.  The top pool stays in
// registers; the pools below it lie in the caller's workspace as [depth][R] planes, so the lanes of a wave that stand at the
// same depth touch one line.  The noise-constrained search (csrc/deconv_search_math.h) and the fit of a baseline
// (csrc/deconv_base_math.h) run that forward pass once or twice a round, with the searched parameter and the baseline in the device
// arrays the pass reads anyway, and between two passes one launch of the sweep kernel, which folds the residual of the stacks and
// moves every trace's bracket or baseline: nothing is read back.  There are two models, DcAr1 (csrc/deconv_math.h) and DcAr2
// (csrc/deconv_ar2_math.h, "A rise time in the deconvolution": pools that carry two data moments and lie in five planes), and one
// interface to them: the pool type, its planes, mu, fresh, push, calc and spike.  The stack view, the forward kernel, the fill, the
// sweep and the host drivers below are each written once against it; a kernel is instantiated per model source (Ar1From<Each>,
// Ar2From), and the launches pick the instantiation from what Args names.  Nothing here may be contracted or reassociated: the
// pragma of deconv_math.h and the per-file flag in _build.py.
#pragma clang fp contract(off)
#include <type_traits>
#include <vector>

#include "common.h"
#include "deconv_math.h"
#include "deconv_search_math.h"
#include "deconv_base_math.h"
#include "deconv_ar2_math.h"
#include "trace_matrix.h"

namespace {

const int kLanes = 64;                       // traces per workgroup: one wave, one lane per trace
const int kFrames = 64;                      // frames per staged tile
const int kPitch = kFrames + 1;              // elements per tile row: lane l reads word l * 65 + k, one bank each (float), two (double)
const int kFillThreads = 256;
const int kSearchThreads = DC_DYN_LANES;     // the sweep: one thread per lane of the fold
const int kSearchMaxGroups = 8192;           // DC_TRACE_DECONV_SEARCH_MAX_GROUPS: beyond, a workgroup walks several traces

// The workspace: planes of R * T 8-byte words, pool i of trace r at word i * R + r of each.  Only the forward kernels store.  What
// the AR(1) and the AR(2) stacks share: the plane of (t0, l), which follows the planes of doubles, and the search in it.
struct StackIndex {
  int2* tl;                                  // (t0, l)
  long R;
  __device__ __forceinline__ StackIndex(const double* ws, int doubles, int R_, long T)
      : tl(reinterpret_cast<int2*>(const_cast<double*>(ws) + doubles * ((long)R_ * T))), R(R_) {}
  __device__ __forceinline__ long at(int32_t i, long r) const { return (long)i * R + r; }
  // The pool of trace r that holds frame t: the last whose start is <= t.  The starts ascend, so a bisection finds it; pool lo
  // starts at or before t, pool hi + 1 (if any) after it.  t in the caller's own integer type: the comparison stays as wide as it
  // was there.
  template <typename Frame>
  __device__ __forceinline__ int32_t pool_of(long r, int32_t lo, int32_t hi, Frame t) const {
    while (lo < hi) {
      const int32_t mid = lo + (hi - lo + 1) / 2;                    // lo < mid <= hi
      if (tl[at(mid, r)].x <= t) lo = mid;
      else hi = mid - 1;
    }
    return lo;
  }
};

// The stacks of a model: Model::kPlanes planes of doubles, the fields of its pool in the order of Model::words -- v and w for AR(1);
// v, u, A and B for AR(2), where v could be had again from A, u and l and is kept, a load for a division --, then (t0, l).
template <class Model>
struct StackView : StackIndex {
  using Pool = typename Model::Pool;
  double* d[Model::kPlanes];
  __device__ __forceinline__ StackView(const double* ws, int R_, long T) : StackIndex(ws, Model::kPlanes, R_, T) {
    for (int j = 0; j < Model::kPlanes; ++j) d[j] = const_cast<double*>(ws) + j * ((long)R_ * T);
  }
  __device__ __forceinline__ Pool load(int32_t i, long r) const {
    Pool p;
    const long word = at(i, r);                                      // once, before the visitor: formed inside it, 8 - 12 VGPRs more in the forward kernels
    Model::words(p, [&](int j, double& x) { x = d[j][word]; });
    const int2 x = tl[word];
    p.t0 = x.x;
    p.l = x.y;
    return p;
  }
  __device__ __forceinline__ void store(int32_t i, long r, const Pool& p) const {
    const long word = at(i, r);
    Model::words(p, [&](int j, const double& x) { d[j][word] = x; });
    tl[word] = make_int2(p.t0, p.l);
  }
  // what a pool's calcium is computed from (Model::calc): the fields that are not used are not loaded
  __device__ __forceinline__ void value(int32_t i, long r, double& val, double& below) const {
    const Pool p = load(i, r);
    val = p.v;
    below = Model::below(p);
  }
};

// the stack of one trace, as dc_deconv_push and dc_ar2_push take it
template <class Model>
struct DeviceStack {
  StackView<Model> s;
  long r;
  __device__ __forceinline__ typename Model::Pool load(int32_t i) const { return s.load(i, r); }
  __device__ __forceinline__ void store(int32_t i, const typename Model::Pool& p) { s.store(i, r, p); }
};

// The walk of a workgroup of one wave over its 64 traces: a tile of 64 traces x 64 frames at a time is staged through `tile`
// (kLanes * kPitch elements of LDS) with coalesced row reads, then lane `lane` walks its own row of the tile, frame(t, y[r][t])
// in ascending t, where its trace exists.  Rows r >= R and frames t >= T of a ragged tile are neither read nor written.
template <typename In, class F>
__device__ __forceinline__ void walk_tiles(In* tile, const In* __restrict__ y, long ld, int R, long T, F frame) {
  const int lane = threadIdx.x;
  const long r0 = (long)blockIdx.x * kLanes;
  const bool mine = r0 + lane < R;
  const int rows = R - r0 < kLanes ? (int)(R - r0) : kLanes;
  for (long f0 = 0; f0 < T; f0 += kFrames) {
    const int frames = T - f0 < kFrames ? (int)(T - f0) : kFrames;
    __syncthreads();                                                 // the previous tile has been consumed
    if (lane < frames) {
#pragma unroll 8
      for (int j = 0; j < rows; ++j) tile[j * kPitch + lane] = y[(r0 + j) * ld + f0 + lane];
    }
    __syncthreads();
    if (mine) {
      for (int k = 0; k < frames; ++k) frame(f0 + k, (double)tile[lane * kPitch + k]);
    }
  }
}

// Where a kernel's model comes from: what the call gave, as the launches pass it on.  of(r): the model of trace r for the forward
// pass and the fill; a lane without a trace (mine = false) reads nothing.  of_table(r): the same for the sweep, whose entry points
// are given the table alone.
// AR(1): one decay g and one table G for all traces (Each = false; gs == nullptr, ldG == 0), or trace r has the decay gs[r] and the
// table row G + r * ldG (Each = true); the arithmetic of a trace is the same, only where its g and G come from.
struct Ar1Args {
  double g;
  const double *gs, *G;
  long ldG;
};
template <bool Each>
struct Ar1From : Ar1Args {
  using Model = DcAr1;
  __device__ __forceinline__ DcAr1 of(long r, bool mine = true) const {
    return {Each ? (mine ? gs[r] : 0.5) : g, Each && mine ? G + r * ldG : G};
  }
  __device__ __forceinline__ DcAr1 of_table(long r) const {
    const double* row = Each ? G + r * ldG : G;
    return {row[1], row};                                            // T >= 1: the table has the entry
  }
};
// AR(2): one pair of coefficients and one table H of three rows of stride ldH for all traces
struct Ar2Args {
  double g1, g2;
  const double* H;
  long ldH;
};
struct Ar2From : Ar2Args {
  using Model = DcAr2;
  __device__ __forceinline__ DcAr2 of(long, bool = true) const { return dc_ar2_model(g1, g2, H, ldH); }
  __device__ __forceinline__ DcAr2 of_table(long r) const { return of(r); }
};

// The forward pass: one workgroup of one wave per 64 traces (walk_tiles), one lane per trace, the model from `from`.
// Base = true: the baseline base[r] leaves every frame of trace r before the penalty's shift (csrc/deconv_base_math.h).
template <typename In, class From, bool Base>
__global__ __launch_bounds__(kLanes) void deconv_forward_kernel(const In* __restrict__ y, long ld, int R, long T, const From from,
                                                               const double* __restrict__ lam, const double* __restrict__ smin,
                                                               const double* __restrict__ base, double* ws, int* __restrict__ pools) {
  using Model = typename From::Model;
  __shared__ In tile[kLanes * kPitch];
  const long r = (long)blockIdx.x * kLanes + threadIdx.x;
  const bool mine = r < R;
  DeviceStack<Model> st = {StackView<Model>(ws, R, T), r};
  const double la = mine ? lam[r] : 0.0, sm = mine ? smin[r] : 0.0;
  const Model m = from.of(r, mine);
  const double b = Base && mine ? base[r] : 0.0;
  typename Model::Pool top = Model::fresh();
  int32_t n = 0;
  walk_tiles(tile, y, ld, R, T, [&](long t, double y_t) {
    const double x = (Base ? dc_base_data(y_t, b) : y_t) - m.mu(la, t, T);
    m.push(top, n, st, x, t, sm);
  });
  if (mine) {
    st.store(n - 1, top);                                            // T >= 1: n >= 1.  The fill kernel reads the workspace only
    pools[r] = n;
  }
}

// One thread per sample (r, t): pool_of over the trace's n pools.  Every output element is written: the calcium by Model::calc, the
// spike, at the first frame of a pool above another, by Model::spike from that pool.
template <class From>
__global__ __launch_bounds__(kFillThreads) void deconv_fill_kernel(const double* __restrict__ ws, const int* __restrict__ pools, int R, long T,
                                                                  const From from, double* __restrict__ calcium, double* __restrict__ spikes) {
  using Model = typename From::Model;
  const long idx = (long)blockIdx.x * kFillThreads + threadIdx.x;
  if (idx >= (long)R * T) return;
  const long r = idx / T;
  const int32_t t = (int32_t)(idx - r * T);
  const Model m = from.of(r);
  const StackView<Model> st(ws, R, T);
  const int32_t lo = st.pool_of(r, 0, pools[r] - 1, t);
  const int32_t k = t - st.tl[st.at(lo, r)].x;
  double val, below;
  st.value(lo, r, val, below);
  const double c = m.calc(val, below, k);
  double s = 0.0;
  if (k == 0 && lo > 0) s = m.spike(c, st.load(lo - 1, r));
  calcium[idx] = c;
  spikes[idx] = s;
}

// ---- the sweep over the stacks: the noise-constrained search (csrc/deconv_search_math.h), the baseline (csrc/deconv_base_math.h) ----
// The state of the searches: planes of R 8-byte words -- lo, hi, rss_lo, target (doubles), phase (an integer): five for the plain
// search; the joint search has two more, b (carried) and b_lo.
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
  __device__ __forceinline__ DcBaseSearch load_joint(long r) const {
    DcBaseSearch q;
    q.s = load(r);
    q.b = w[5 * R + r];
    q.b_lo = w[6 * R + r];
    return q;
  }
  __device__ __forceinline__ void store(long r, const DcBaseSearch& q) {
    store(r, q.s);
    w[5 * R + r] = q.b;
    w[6 * R + r] = q.b_lo;
  }
};

// one thread per trace: the state before round 0 (Base: base holds b_0 and stays), and round 0's parameter
template <bool Base>
__global__ __launch_bounds__(kSearchThreads) void deconv_begin_kernel(const double* __restrict__ sigma, const double* __restrict__ base, int R,
                                                                      long T, double* state, double* __restrict__ param) {
  const long r = (long)blockIdx.x * kSearchThreads + threadIdx.x;
  if (r >= R) return;
  SearchState st = {state, (long)R};
  if constexpr (Base) st.store(r, dc_base_search_begin(sigma[r], T, base[r]));
  else st.store(r, dc_search_begin(sigma[r], T));
  param[r] = 0.0;
}

// What thread 0 does with the folds of a trace, and where it writes: `mode` is DC_BASE_*; state, param, rss and status are not
// touched in the mode DC_BASE_FIT; base belongs to the sweeps with a baseline; sums, where given, takes their three folds as planes
// of R doubles.
struct SweepOut {
  int mode;
  double* state;
  double* param;
  double* base;
  double* rss;
  int* status;
  double* sums;
};

// The pool that holds the frame a thread of the sweep stands at: pool `at` of the trace, frames [start, end), and the two words
// Model::calc takes, its value and what lies below it.  A thread's frames ascend, so it seeks from its previous pool upwards, and
// only when a frame t >= end has left that pool.
struct PoolCursor {
  int32_t at = 0, start = 0, end = 0;        // no pool yet: frame 0 seeks
  double val = 0.0, below = 0.0;
  __device__ __forceinline__ int32_t length() const { return end - start; }
  template <class View>
  __device__ __forceinline__ void seek(const View& st, long r, int32_t n, long t) {
    at = st.pool_of(r, at, n - 1, t);
    const int2 own = st.tl[st.at(at, r)];
    start = own.x;
    end = own.x + own.y;
    st.value(at, r, val, below);
  }
};

// thread 0 of the plain search: one step on RSS(p); the bracket moves and the next parameter is written (the last pass: p*, RSS(p*)
// and the status instead)
__device__ __forceinline__ void search_tail(const SweepOut& o, long r, long R, double RSS) {
  SearchState st = {o.state, R};
  DcSearch q = st.load(r);
  const double next = dc_search_step(q, o.param[r], RSS);
  st.store(r, q);
  if (o.mode == DC_BASE_PASS_LAST) {
    o.param[r] = q.lo;
    o.rss[r] = q.rss_lo;
    o.status[r] = dc_search_status(q);
  } else {
    o.param[r] = next;
  }
}

// thread 0 of the sweeps with a baseline b: the baseline step (DC_BASE_FIT; DC_BASE_PASS_A, which also keeps it in the state) or the
// step of the joint search (DC_BASE_PASS_B; DC_BASE_PASS_LAST writes p*, b*, the residual and the status)
__device__ __forceinline__ void base_tail(const SweepOut& o, long r, long R, long T, double b, double RSS, double S, double A) {
  if (o.sums) {
    o.sums[r] = RSS;
    o.sums[R + r] = S;
    o.sums[2 * R + r] = A;
  }
  if (o.mode == DC_BASE_FIT) {
    o.base[r] = dc_base_step(b, S, A, T);
    return;
  }
  SearchState st = {o.state, R};
  DcBaseSearch x = st.load_joint(r);
  if (o.mode == DC_BASE_PASS_A) {
    o.base[r] = dc_base_search_newton(x, S, A, T);
    st.store(r, x);
    return;
  }
  const double next = dc_base_search_step(x, o.param[r], RSS);
  st.store(r, x);
  if (o.mode == DC_BASE_PASS_LAST) {
    o.param[r] = x.s.lo;
    o.base[r] = x.b_lo;
    o.rss[r] = x.s.rss_lo;
    o.status[r] = dc_search_status(x.s);
  } else {
    o.param[r] = next;
  }
}

// The folds of the stacks the forward pass left in the workspace, then thread 0's turn.  One workgroup of 256 threads per trace (at
// most 8192 workgroups: beyond, a workgroup walks several traces): thread j owns lane j of every fold, t = j, j + 256, ... (coalesced
// reads of y), each lane sum s = s + term in ascending t from +0.0; the pool of t is found as the fill kernel finds it, through the
// thread's PoolCursor.  Base = false folds the residual term of the plain search into red[256]; Base = true takes the baseline
// base[r] off the data and folds RSS, S and A of deconv_base_math.h into red[3 * 256].  The tree through LDS is dc_dyn_fold_tree of
// trace_dyn_math.h.  Its results red[0], red[256] and red[512] are thread 0's own words, and its last barrier frees the others for
// the next trace; it also lies between every thread's read of base[r] and thread 0's write.  Every word has one writer; frames
// t >= T of a row and rows r >= R are never read.  The model comes from the table (From::of_table), the calcium of a frame from
// Model::calc.  The sweep with a baseline exists for AR(1) only: dc_base_gain is the arithmetic of one decay.
template <class Model, bool Base>
constexpr bool kSweepExists = !Base || std::is_same<Model, DcAr1>::value;

template <typename In, class From, bool Base>
__global__ __launch_bounds__(kSearchThreads) void deconv_sweep_kernel(const In* __restrict__ y, long ld, int R, long T, const From from,
                                                                      const double* __restrict__ ws, const int* __restrict__ pools,
                                                                      const SweepOut out) {
  using Model = typename From::Model;
  static_assert(kSweepExists<Model, Base>, "the sweep with a baseline is AR(1) arithmetic");
  const int folds = Base ? 3 : 1;
  __shared__ double red[folds * kSearchThreads];
  const int tid = threadIdx.x;
  const StackView<Model> st(ws, R, T);
  for (long r = blockIdx.x; r < R; r += gridDim.x) {
    const In* __restrict__ row = y + r * ld;
    const Model m = from.of_table(r);
    const double b = Base ? out.base[r] : 0.0;
    const int32_t n = pools[r];
    PoolCursor pool;
    double Gl = 1.0;
    double q = 0.0, s = 0.0, a = 0.0;
    for (long t = tid; t < T; t += kSearchThreads) {
      if (t >= pool.end) {
        pool.seek(st, r, n, t);
        if constexpr (Base) Gl = m.G[pool.length()];
      }
      const double c = m.calc(pool.val, pool.below, (int32_t)(t - pool.start));
      if constexpr (Base) {
        const double d = dc_base_resid((double)row[t], b, c);
        q = q + d * d;
        s = s + d;
        a = a + dc_base_gain_at(pool.val, t, pool.start, m.g, Gl);
      } else {
        q = q + dc_search_term((double)row[t], c);
      }
    }
    red[tid] = q;
    if constexpr (Base) {
      red[kSearchThreads + tid] = s;
      red[2 * kSearchThreads + tid] = a;
    }
    dc_dyn_fold_tree(red, folds);
    if (tid == 0) {
      if constexpr (Base) base_tail(out, r, R, T, b, red[0], red[kSearchThreads], red[2 * kSearchThreads]);
      else search_tail(out, r, R, red[0]);
    }
  }
}

// ---- the launches: the arguments have been checked -----------------------------------------------------------------------------------
// What every launch of a call shares: the model it named and that model's description (the other one is empty); base == nullptr: no
// baseline, the kernels of the entry points that have none.
enum ModelKind { kAr1, kAr2 };
struct Args {
  const char* who;
  const void* y;
  int is_f64;
  long ld;
  int R;
  long T;
  ModelKind model;
  Ar1Args ar1;
  Ar2Args ar2;
  const double *lam, *smin, *base;
  void* ws;
  int* pools;
  dc_stream_t stream;
};

// a flag of the call as a template argument of its kernel: launch(std::true_type()) or launch(std::false_type())
template <class F>
void with_flag(bool flag, F launch) {
  if (flag) launch(std::true_type());
  else launch(std::false_type());
}

// where the kernels of the call take their model from: launch(from), an Ar1From<Each> or an Ar2From
template <class F>
void with_model_of(const Args& a, F launch) {
  if (a.model == kAr2) launch(Ar2From{a.ar2});
  else with_flag(a.ar1.ldG != 0, [&](auto each) { launch(Ar1From<decltype(each)::value>{a.ar1}); });
}

// In, the model and Base of the forward and sweep kernels from the call: launch(In(), from, base), base as with_flag gives it
template <class F>
void with_kernel_of(const Args& a, F launch) {
  with_model_of(a, [&](auto from) {
    with_flag(a.base != nullptr, [&](auto base) {
      if (a.is_f64) launch(double(), from, base);
      else launch(float(), from, base);
    });
  });
}

int launch_forward(const Args& a) {
  const unsigned groups = (unsigned)(((long)a.R + kLanes - 1) / kLanes);                    // <= 2^25: no cap
  with_kernel_of(a, [&](auto in, auto from, auto base) {
    using In = decltype(in);
    hipLaunchKernelGGL((deconv_forward_kernel<In, decltype(from), decltype(base)::value>), dim3(groups), dim3(kLanes), 0, (hipStream_t)a.stream,
                       (const In*)a.y, a.ld, a.R, a.T, from, a.lam, a.smin, a.base, (double*)a.ws, a.pools);
  });
  DC_CHECK_LAUNCH(a.who);
  return DC_OK;
}

// the forward pass, then the fill
int launch_deconv(const Args& a, double* calcium, double* spikes) {
  const int rc = launch_forward(a);
  if (rc != DC_OK) return rc;
  const unsigned blocks = (unsigned)(((long)a.R * a.T + kFillThreads - 1) / kFillThreads);  // <= 2^23: no cap
  with_model_of(a, [&](auto from) {
    hipLaunchKernelGGL(deconv_fill_kernel<decltype(from)>, dim3(blocks), dim3(kFillThreads), 0, (hipStream_t)a.stream, (const double*)a.ws, a.pools,
                       a.R, a.T, from, calcium, spikes);
  });
  DC_CHECK_LAUNCH(a.who);
  return DC_OK;
}

// the folds of the stacks in ws and what out.mode does with them
int launch_sweep(const Args& a, const SweepOut& out) {
  const unsigned groups = (unsigned)(a.R < kSearchMaxGroups ? a.R : kSearchMaxGroups);
  DC_REQUIRE(a.model == kAr1 || a.base == nullptr, DC_EUNSUP, "%s: the AR(2) sweep takes no baseline", a.who);
  with_kernel_of(a, [&](auto in, auto from, auto base) {
    using In = decltype(in);
    using From = decltype(from);
    constexpr bool kBase = decltype(base)::value;
    if constexpr (kSweepExists<typename From::Model, kBase>) {      // else: refused above
      hipLaunchKernelGGL((deconv_sweep_kernel<In, From, kBase>), dim3(groups), dim3(kSearchThreads), 0, (hipStream_t)a.stream, (const In*)a.y, a.ld,
                         a.R, a.T, from, (const double*)a.ws, a.pools, out);
    }
  });
  DC_CHECK_LAUNCH(a.who);
  return DC_OK;
}

// one pass: the forward pass, then the sweep over the stacks it left
int launch_pass(const Args& a, const SweepOut& out) {
  const int rc = launch_forward(a);
  return rc != DC_OK ? rc : launch_sweep(a, out);
}

// `rounds` baseline steps, then the forward pass and the fill at b_N
int launch_fit_base(const Args& a, int rounds, double* base, double* calcium, double* spikes) {
  for (int round = 0; round < rounds; ++round) {
    const int rc = launch_pass(a, {DC_BASE_FIT, nullptr, nullptr, base, nullptr, nullptr, nullptr});
    if (rc != DC_OK) return rc;
  }
  return launch_deconv(a, calcium, spikes);
}

// The search: round 0, the rounds and the final pass.  out.param is the array the forward passes read the searched parameter from,
// `other` the fixed one.  With a baseline to fit (a.base, which is out.base) a round is two passes: pass A, the baseline step at
// (p, b), then pass B, the search step on RSS at (p, b').
int launch_constrained(Args a, int which, const double* sigma, const double* other, int rounds, SweepOut out, double* calcium, double* spikes) {
  a.lam = which == DC_SEARCH_LAM ? out.param : other;
  a.smin = which == DC_SEARCH_LAM ? other : out.param;
  const unsigned begin = (unsigned)(((long)a.R + kSearchThreads - 1) / kSearchThreads);
  with_flag(a.base != nullptr, [&](auto base) {
    hipLaunchKernelGGL(deconv_begin_kernel<decltype(base)::value>, dim3(begin), dim3(kSearchThreads), 0, (hipStream_t)a.stream, sigma, a.base, a.R,
                       a.T, out.state, out.param);
  });
  DC_CHECK_LAUNCH(a.who);
  for (int round = 0; round <= rounds; ++round) {
    if (a.base && round > 0) {
      out.mode = DC_BASE_PASS_A;
      const int rc = launch_pass(a, out);
      if (rc != DC_OK) return rc;
    }
    out.mode = round == rounds ? DC_BASE_PASS_LAST : DC_BASE_PASS_B;
    const int rc = launch_pass(a, out);
    if (rc != DC_OK) return rc;
  }
  return launch_deconv(a, calcium, spikes);
}

// ---- the checks the entry points share ----------------------------------------------------------------------------------------------
int check_limits(const char* who, int R, long T, double g) {
  DC_REQUIRE(g > 0.0 && g < 1.0, DC_EINVAL, "%s: g = %g is outside (0, 1)", who, g);      // a NaN fails both comparisons
  return dc_trace_check_limits(who, R, T);
}

// what the device entry points with a decay per trace or one for all share
int check_decay(const char* who, int R, long T, double g, const double* gs, long ldG) {
  if (gs) DC_REQUIRE(ldG >= T + 1, DC_EINVAL, "%s: ldG = %ld is below T + 1 = %ld", who, ldG, T + 1);
  return check_limits(who, R, T, gs ? 0.5 : g);                      // per trace, the decays lie in device memory: THE CALLER PROMISES 0 < gs[r] < 1
}

// ldG of the entry points that take a table and no decay: 0, one table for all traces, or the stride of one row per trace
int check_table_stride(const char* who, long ldG, long T) {
  DC_REQUIRE(ldG == 0 || ldG >= T + 1, DC_EINVAL, "%s: ldG = %ld is neither 0 nor at least T + 1 = %ld", who, ldG, T + 1);
  return DC_OK;
}

int check_search(const char* who, int which, int rounds) {
  DC_REQUIRE(which == DC_SEARCH_SMIN || which == DC_SEARCH_LAM, DC_EINVAL, "%s: which = %d is neither 0 (smin) nor 1 (lam)", who, which);
  DC_REQUIRE(rounds >= 1 && rounds <= DC_SEARCH_MAX_ROUNDS, DC_EINVAL, "%s: rounds = %d is outside [1, %d]", who, rounds, DC_SEARCH_MAX_ROUNDS);
  return DC_OK;
}

// ---- the host entry points: one trace at a time through the host restatements of the three headers ----------------------------------
// The ranges of what a host entry point reads per trace, trace by trace; an array the entry point does not take is nullptr (lam goes
// with smin, sigma with other).
int check_host_ranges(const char* who, int R, const double* lam, const double* smin, const double* sigma, const double* other, const double* base) {
  for (int r = 0; r < R; ++r) {
    if (lam) DC_REQUIRE(lam[r] >= 0.0 && smin[r] >= 0.0, DC_EINVAL, "%s: trace %d: lam = %g, smin = %g: neither may be negative", who, r, lam[r], smin[r]);
    if (sigma) {
      DC_REQUIRE(sigma[r] >= 0.0 && sigma[r] < 0x1p500, DC_EINVAL, "%s: trace %d: sigma = %g is outside [0, 2^500)", who, r, sigma[r]);
      DC_REQUIRE(other[r] >= 0.0, DC_EINVAL, "%s: trace %d: the fixed parameter %g is negative", who, r, other[r]);
    }
    if (base) DC_REQUIRE(base[r] - base[r] == 0.0, DC_EINVAL, "%s: trace %d: the baseline %g is not finite", who, r, base[r]);
  }
  return DC_OK;
}

// the one table of the host entry points that take no ldG: it holds the decay; R, T >= 1
int check_host_table(const char* who, int R, long T, const double* G) {
  DC_REQUIRE(G[0] == 1.0, DC_EINVAL, "%s: G[0] = %g is not 1", who, G[0]);
  return check_limits(who, R, T, G[1]);
}

// the AR(1) model of trace r on the host: one table for all (ldG == 0) or row r; -> DC_OK where the row holds a decay
struct HostAr1 {
  const char* who;
  const double* G;
  long ldG;
  int operator()(int r, DcAr1& m) const {
    m.G = G + (long)r * ldG;
    DC_REQUIRE(m.G[0] == 1.0, DC_EINVAL, "%s: trace %d: G[0] = %g is not 1", who, r, m.G[0]);
    m.g = m.G[1];
    DC_REQUIRE(m.g > 0.0 && m.g < 1.0, DC_EINVAL, "%s: trace %d: g = %g is outside (0, 1)", who, r, m.g);
    return DC_OK;
  }
};

// the AR(2) model of every trace: checked before the rows
struct HostAr2 {
  DcAr2 m;
  int operator()(int, DcAr2& out) const {
    out = m;
    return DC_OK;
  }
};

// one trace of a host entry point: its row and model, and the scratch of the header functions (T pools, T doubles twice)
template <class Model, typename Row>
struct HostTrace {
  int r;
  Row y;                                     // const float* or const double*
  Model m;
  std::vector<typename Model::Pool>& pool;
  double* c;
  double* a;
};

// what the outputs of a trace are computed at
struct HostFit {
  double lam, smin, b;
};

// after a search: p, the value found for the parameter `which`, beside the fixed one
HostFit host_fit_found(int which, double p, double other, double b) {
  if (which == DC_SEARCH_LAM) return {p, other, b};
  return {other, p, b};
}

// The rows of a host entry point; R, T >= 1.  model_of(r, m) gives trace r its model or refuses it.  fit(h), a generic lambda, gets
// trace h.r with its row as the type it has, does what the entry point does before the outputs and returns what they -- calcium,
// spikes and the pool count -- are computed at.
template <class Model, class Of, class F>
int host_rows(const void* y, int is_f64, long ld, int R, long T, Of model_of, double* calcium, double* spikes, int* pools, F fit) {
  std::vector<typename Model::Pool> pool((size_t)T);
  std::vector<double> scratch(2 * (size_t)T);
  for (int r = 0; r < R; ++r) {
    Model m;
    const int rc = model_of(r, m);
    if (rc != DC_OK) return rc;
    double *c = calcium + (long)r * T, *s = spikes + (long)r * T;
    auto one = [&](auto row) {
      const HostTrace<Model, decltype(row)> h = {r, row, m, pool, scratch.data(), scratch.data() + T};
      const HostFit at = fit(h);
      const int32_t n = dc_forward_host(row, T, m, at.lam, at.smin, at.b, pool);
      pools[r] = n;
      dc_calcium_host(pool, n, m, c);
      dc_spikes_host(pool, n, m, T, c, s);
    };
    if (is_f64) one((const double*)y + (long)r * ld);
    else one((const float*)y + (long)r * ld);
  }
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
  rc = check_decay(who, R, T, g, nullptr, 0);
  if (rc != DC_OK) return rc;
  DC_REQUIRE(dc_aligned(7, G, lam, smin, ws, calcium, spikes) && dc_aligned(3, pools) && dc_trace_aligned(y, is_f64), DC_EINVAL, "%s: misaligned buffer", who);
  if (R == 0 || T == 0) return DC_OK;
  return launch_deconv({who, y, is_f64, ld, R, T, kAr1, {g, nullptr, G, 0}, {}, lam, smin, nullptr, ws, pools, stream}, calcium, spikes);
}

extern "C" int dc_trace_deconv_ar1_each(const void* y, int is_f64, long ld, int R, long T, const double* g, const double* G, long ldG,
                                        const double* lam, const double* smin, void* ws, double* calcium, double* spikes, int* pools,
                                        dc_stream_t stream) {
  const char* who = "dc_trace_deconv_ar1_each";
  DC_REQUIRE(g && G && lam && smin && ws && calcium && spikes && pools, DC_EINVAL, "%s: null pointer", who);
  int rc = dc_trace_check_counts(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  rc = check_decay(who, R, T, 0.0, g, ldG);
  if (rc != DC_OK) return rc;
  DC_REQUIRE(dc_aligned(7, g, G, lam, smin, ws, calcium, spikes) && dc_aligned(3, pools) && dc_trace_aligned(y, is_f64), DC_EINVAL, "%s: misaligned buffer", who);
  if (R == 0 || T == 0) return DC_OK;
  return launch_deconv({who, y, is_f64, ld, R, T, kAr1, {0.0, g, G, ldG}, {}, lam, smin, nullptr, ws, pools, stream}, calcium, spikes);
}

extern "C" int dc_trace_deconv_ar1_host(const void* y, int is_f64, long ld, int R, long T, const double* G, const double* lam,
                                        const double* smin, double* calcium, double* spikes, int* pools) {
  const char* who = "dc_trace_deconv_ar1_host";
  DC_REQUIRE(G && lam && smin && calcium && spikes && pools, DC_EINVAL, "%s: null pointer", who);
  DC_REQUIRE(dc_aligned(7, G, lam, smin, calcium, spikes) && dc_aligned(3, pools) && dc_trace_aligned(y, is_f64), DC_EINVAL, "%s: misaligned buffer", who);
  int rc = dc_trace_check_counts(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  if (R == 0 || T == 0) return DC_OK;                                // G is not read: without frames it need not hold g
  rc = check_host_table(who, R, T, G);
  if (rc != DC_OK) return rc;
  rc = check_host_ranges(who, R, lam, smin, nullptr, nullptr, nullptr);
  if (rc != DC_OK) return rc;
  return host_rows<DcAr1>(y, is_f64, ld, R, T, HostAr1{who, G, 0}, calcium, spikes, pools, [&](const auto& h) { return HostFit{lam[h.r], smin[h.r], 0.0}; });
}

// ---- the noise-constrained search --------------------------------------------------------------------------------------------------
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
  rc = check_decay(who, R, T, g, gs, ldG);
  if (rc != DC_OK) return rc;                                        // sigma, fixed_other likewise: THE CALLER PROMISES 0 <= sigma[r] < 2^500, finite, and fixed_other[r] >= 0
  DC_REQUIRE(dc_aligned(7, gs, G, sigma, fixed_other, ws, state, calcium, spikes, param, rss) && dc_aligned(3, pools, status) &&
                 dc_trace_aligned(y, is_f64),
             DC_EINVAL, "%s: misaligned buffer", who);
  if (R == 0 || T == 0) return DC_OK;
  return launch_constrained({who, y, is_f64, ld, R, T, kAr1, {g, gs, G, gs ? ldG : 0}, {}, nullptr, nullptr, nullptr, ws, pools, stream}, which, sigma, fixed_other,
                            rounds, {0, (double*)state, param, nullptr, rss, status, nullptr}, calcium, spikes);
}

extern "C" int dc_trace_deconv_search_step(const void* y, int is_f64, long ld, int R, long T, const double* G, long ldG, const void* ws,
                                           const int* pools, int last, void* state, double* param, double* rss, int* status,
                                           dc_stream_t stream) {
  const char* who = "dc_trace_deconv_search_step";
  DC_REQUIRE(G && ws && pools && state && param && rss && status, DC_EINVAL, "%s: null pointer", who);
  int rc = dc_trace_check_counts(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  DC_REQUIRE(last == 0 || last == 1, DC_EINVAL, "%s: last = %d is neither 0 nor 1", who, last);
  rc = check_table_stride(who, ldG, T);
  if (rc != DC_OK) return rc;
  rc = dc_trace_check_limits(who, R, T);
  if (rc != DC_OK) return rc;
  DC_REQUIRE(dc_aligned(7, G, ws, state, param, rss) && dc_aligned(3, pools, status) && dc_trace_aligned(y, is_f64), DC_EINVAL, "%s: misaligned buffer", who);
  if (R == 0 || T == 0) return DC_OK;
  // the sweep only reads ws and pools
  return launch_sweep({who, y, is_f64, ld, R, T, kAr1, {0.0, nullptr, G, ldG}, {}, nullptr, nullptr, nullptr, const_cast<void*>(ws), const_cast<int*>(pools), stream},
                      {last ? DC_BASE_PASS_LAST : DC_BASE_PASS_B, (double*)state, param, nullptr, rss, status, nullptr});
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
  rc = check_host_table(who, R, T, G);
  if (rc != DC_OK) return rc;
  rc = check_host_ranges(who, R, nullptr, nullptr, sigma, fixed_other, nullptr);
  if (rc != DC_OK) return rc;
  return host_rows<DcAr1>(y, is_f64, ld, R, T, HostAr1{who, G, 0}, calcium, spikes, pools, [&](const auto& h) {
    const int r = h.r;
    dc_search_host(h.y, T, h.m, which, sigma[r], fixed_other[r], rounds, h.pool, h.c, param + r, rss + r, status + r);
    return host_fit_found(which, param[r], fixed_other[r], 0.0);
  });
}

// ---- a baseline in the deconvolution (csrc/deconv_base_math.h) -----------------------------------------------------------------------
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
  return launch_deconv({who, y, is_f64, ld, R, T, kAr1, {g, gs, G, gs ? ldG : 0}, {}, lam, smin, base, ws, pools, stream}, calcium, spikes);
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
  return launch_fit_base({who, y, is_f64, ld, R, T, kAr1, {g, gs, G, gs ? ldG : 0}, {}, lam, smin, base, ws, pools, stream}, rounds, base, calcium, spikes);
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
  return launch_constrained({who, y, is_f64, ld, R, T, kAr1, {g, gs, G, gs ? ldG : 0}, {}, nullptr, nullptr, base, ws, pools, stream}, which, sigma, fixed_other,
                            rounds, {0, (double*)state, param, base, rss, status, nullptr}, calcium, spikes);
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
  rc = check_table_stride(who, ldG, T);
  if (rc != DC_OK) return rc;
  rc = dc_trace_check_limits(who, R, T);
  if (rc != DC_OK) return rc;
  DC_REQUIRE(dc_aligned(7, G, ws, state, param, base, rss, sums) && dc_aligned(3, pools, status) && dc_trace_aligned(y, is_f64), DC_EINVAL,
             "%s: misaligned buffer", who);
  if (R == 0 || T == 0) return DC_OK;
  // the sweep only reads ws and pools
  return launch_sweep({who, y, is_f64, ld, R, T, kAr1, {0.0, nullptr, G, ldG}, {}, nullptr, nullptr, base, const_cast<void*>(ws), const_cast<int*>(pools), stream},
                      {mode, (double*)state, param, base, rss, status, sums});
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
  rc = check_table_stride(who, ldG, T);
  if (rc != DC_OK) return rc;
  if (R == 0 || T == 0) return DC_OK;                                // G is not read: without frames it need not hold g
  rc = dc_trace_check_limits(who, R, T);
  if (rc != DC_OK) return rc;
  rc = check_host_ranges(who, R, lam, smin, nullptr, nullptr, base);
  if (rc != DC_OK) return rc;
  return host_rows<DcAr1>(y, is_f64, ld, R, T, HostAr1{who, G, ldG}, calcium, spikes, pools, [&](const auto& h) {
    const int r = h.r;
    base[r] = dc_base_fit_host(h.y, T, h.m.g, h.m.G, lam[r], smin[r], base[r], rounds, h.pool, h.c, h.a);
    return HostFit{lam[r], smin[r], base[r]};
  });
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
  rc = check_table_stride(who, ldG, T);
  if (rc != DC_OK) return rc;
  if (R == 0 || T == 0) return DC_OK;                                // G is not read: without frames it need not hold g
  rc = dc_trace_check_limits(who, R, T);
  if (rc != DC_OK) return rc;
  rc = check_host_ranges(who, R, nullptr, nullptr, sigma, fixed_other, base);
  if (rc != DC_OK) return rc;
  return host_rows<DcAr1>(y, is_f64, ld, R, T, HostAr1{who, G, ldG}, calcium, spikes, pools, [&](const auto& h) {
    const int r = h.r;
    dc_base_search_host(h.y, T, h.m.g, h.m.G, which, sigma[r], fixed_other[r], base[r], rounds, h.pool, h.c, h.a, param + r, base + r, rss + r, status + r);
    return host_fit_found(which, param[r], fixed_other[r], base[r]);
  });
}

// ---- a rise time in the deconvolution: AR(2) (csrc/deconv_ar2_math.h) -----------------------------------------------------------------
namespace {

// the coefficients and the table's stride
int check_ar2(const char* who, int R, long T, double g1, double g2, long ldH) {
  DC_REQUIRE(dc_ar2_roots_ok(g1, g2), DC_EINVAL, "%s: g1 = %g, g2 = %g are not those of two real roots 0 < r < d < 1", who, g1, g2);
  DC_REQUIRE(ldH >= T + 1, DC_EINVAL, "%s: ldH = %ld is below T + 1 = %ld", who, ldH, T + 1);
  return dc_trace_check_limits(who, R, T);
}

// the table of a host entry point holds the coefficients; T >= 1
int check_ar2_host_table(const char* who, double g1, const double* H, long ldH) {
  DC_REQUIRE(H[0] == 1.0 && H[1] == g1 && H[ldH] == 0.0 && H[2 * ldH] == 0.0, DC_EINVAL,
             "%s: the table does not begin with h = (1, g1), HH[0] = HP[0] = 0", who);
  return DC_OK;
}

}  // namespace

extern "C" long dc_trace_deconv_ar2_ws_bytes(int R, long T) {
  if (R <= 0 || T <= 0 || T > DC_TRACE_DECONV_MAX_FRAMES || (long)R * T > DC_TRACE_DECONV_MAX_SAMPLES) return 0;
  return 40L * R * T;
}

extern "C" int dc_trace_deconv_ar2(const void* y, int is_f64, long ld, int R, long T, double g1, double g2, const double* H, long ldH,
                                   const double* lam, const double* smin, const double* base, void* ws, double* calcium, double* spikes,
                                   int* pools, dc_stream_t stream) {
  const char* who = "dc_trace_deconv_ar2";
  DC_REQUIRE(H && lam && smin && ws && calcium && spikes && pools, DC_EINVAL, "%s: null pointer", who);
  int rc = dc_trace_check_counts(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  rc = check_ar2(who, R, T, g1, g2, ldH);
  if (rc != DC_OK) return rc;                                        // lam, smin, base: THE CALLER PROMISES lam, smin >= 0 and a finite base
  DC_REQUIRE(dc_aligned(7, H, lam, smin, base, ws, calcium, spikes) && dc_aligned(3, pools) && dc_trace_aligned(y, is_f64), DC_EINVAL,
             "%s: misaligned buffer", who);
  if (R == 0 || T == 0) return DC_OK;
  return launch_deconv({who, y, is_f64, ld, R, T, kAr2, {}, {g1, g2, H, ldH}, lam, smin, base, ws, pools, stream}, calcium, spikes);
}

extern "C" int dc_trace_deconv_ar2_host(const void* y, int is_f64, long ld, int R, long T, double g1, double g2, const double* H, long ldH,
                                        const double* lam, const double* smin, const double* base, double* calcium, double* spikes,
                                        int* pools) {
  const char* who = "dc_trace_deconv_ar2_host";
  DC_REQUIRE(H && lam && smin && calcium && spikes && pools, DC_EINVAL, "%s: null pointer", who);
  DC_REQUIRE(dc_aligned(7, H, lam, smin, base, calcium, spikes) && dc_aligned(3, pools) && dc_trace_aligned(y, is_f64), DC_EINVAL,
             "%s: misaligned buffer", who);
  int rc = dc_trace_check_counts(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  rc = check_ar2(who, R, T, g1, g2, ldH);
  if (rc != DC_OK) return rc;
  if (R == 0 || T == 0) return DC_OK;
  rc = check_ar2_host_table(who, g1, H, ldH);
  if (rc != DC_OK) return rc;
  rc = check_host_ranges(who, R, lam, smin, nullptr, nullptr, base);
  if (rc != DC_OK) return rc;
  return host_rows<DcAr2>(y, is_f64, ld, R, T, HostAr2{dc_ar2_model(g1, g2, H, ldH)}, calcium, spikes, pools,
                          [&](const auto& h) { return HostFit{lam[h.r], smin[h.r], base ? base[h.r] : 0.0}; });
}

extern "C" int dc_trace_deconv_ar2_constrained(const void* y, int is_f64, long ld, int R, long T, double g1, double g2, const double* H, long ldH,
                                               int which, const double* sigma, const double* fixed_other, int rounds, void* ws, void* state,
                                               double* calcium, double* spikes, int* pools, double* param, double* rss, int* status,
                                               dc_stream_t stream) {
  const char* who = "dc_trace_deconv_ar2_constrained";
  DC_REQUIRE(H && sigma && fixed_other && ws && state && calcium && spikes && pools && param && rss && status, DC_EINVAL, "%s: null pointer", who);
  int rc = dc_trace_check_counts(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  rc = check_search(who, which, rounds);
  if (rc != DC_OK) return rc;
  rc = check_ar2(who, R, T, g1, g2, ldH);
  if (rc != DC_OK) return rc;                                        // sigma, fixed_other: THE CALLER PROMISES 0 <= sigma[r] < 2^500, finite, and fixed_other[r] >= 0
  DC_REQUIRE(dc_aligned(7, H, sigma, fixed_other, ws, state, calcium, spikes, param, rss) && dc_aligned(3, pools, status) &&
                 dc_trace_aligned(y, is_f64),
             DC_EINVAL, "%s: misaligned buffer", who);
  if (R == 0 || T == 0) return DC_OK;
  return launch_constrained({who, y, is_f64, ld, R, T, kAr2, {}, {g1, g2, H, ldH}, nullptr, nullptr, nullptr, ws, pools, stream}, which, sigma,
                            fixed_other, rounds, {0, (double*)state, param, nullptr, rss, status, nullptr}, calcium, spikes);
}

extern "C" int dc_trace_deconv_ar2_constrained_host(const void* y, int is_f64, long ld, int R, long T, double g1, double g2, const double* H,
                                                    long ldH, int which, const double* sigma, const double* fixed_other, int rounds,
                                                    double* calcium, double* spikes, int* pools, double* param, double* rss, int* status) {
  const char* who = "dc_trace_deconv_ar2_constrained_host";
  DC_REQUIRE(H && sigma && fixed_other && calcium && spikes && pools && param && rss && status, DC_EINVAL, "%s: null pointer", who);
  DC_REQUIRE(dc_aligned(7, H, sigma, fixed_other, calcium, spikes, param, rss) && dc_aligned(3, pools, status) && dc_trace_aligned(y, is_f64),
             DC_EINVAL, "%s: misaligned buffer", who);
  int rc = dc_trace_check_counts(who, y, is_f64, ld, R, T);
  if (rc != DC_OK) return rc;
  rc = check_search(who, which, rounds);
  if (rc != DC_OK) return rc;
  rc = check_ar2(who, R, T, g1, g2, ldH);
  if (rc != DC_OK) return rc;
  if (R == 0 || T == 0) return DC_OK;
  rc = check_ar2_host_table(who, g1, H, ldH);
  if (rc != DC_OK) return rc;
  rc = check_host_ranges(who, R, nullptr, nullptr, sigma, fixed_other, nullptr);
  if (rc != DC_OK) return rc;
  return host_rows<DcAr2>(y, is_f64, ld, R, T, HostAr2{dc_ar2_model(g1, g2, H, ldH)}, calcium, spikes, pools, [&](const auto& h) {
    const int r = h.r;
    dc_search_host(h.y, T, h.m, which, sigma[r], fixed_other[r], rounds, h.pool, h.c, param + r, rss + r, status + r);
    return host_fit_found(which, param[r], fixed_other[r], 0.0);
  });
}
