// The arithmetic of the AR(1) deconvolution (include/dcunet.h, "Spikes by deconvolution"; csrc/deconv.hip): the push / merge step
// of the pool stack, the two output formulas, the model DcAr1 that names them for the code written once over AR(1) and AR(2) and,
// in a host-only tail, the forward pass and the outputs of one trace under either model.  Plain C++ like
// footprint_math.h, so the same inline functions compile for the device kernels, for the host entry point dc_trace_deconv_ar1_host
// and into a stand-alone host program (tests/native/deconv_math_check.cpp, run under the address / undefined-behaviour sanitizers).
// The result is defined bit for bit:
// IEEE double adds, multiplies, one division per merge and comparisons in the order written here.  No fused multiply-add and no
// reassociation anywhere: the pragma below, and -ffp-contract=off for deconv.hip in _build.py.
#pragma once
#pragma clang fp contract(off)
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DC_DECONV_HD __host__ __device__ inline
#else
#define DC_DECONV_HD inline
#endif

// A pool: `l` consecutive frames from t0 on whose calcium is v G[k], k = 0 .. l - 1; w is the weight of v in a merge.
struct DcPool {
  double v, w;
  int32_t t0, l;
};

// what is subtracted from frame t of a trace of T frames: the L1 penalty lam on the spikes, written as a shift of the data
DC_DECONV_HD double dc_deconv_mu(double lam, double g, long t, long T) { return t < T - 1 ? lam * (1.0 - g) : lam; }

// the frame that the forward pass pushes, before the penalty's shift: the baseline b of deconv_base_math.h leaves the data first
DC_DECONV_HD double dc_base_data(double y, double b) { return y - b; }

DC_DECONV_HD DcPool dc_deconv_new(double x, long t) {
  DcPool q;
  q.v = x;
  q.w = 1.0;
  q.t0 = (int32_t)t;
  q.l = 1;
  return q;
}

// does q, the pool above p, start below what p has decayed to (a = G[p.l]) plus the smallest spike allowed?
DC_DECONV_HD bool dc_deconv_violates(const DcPool& p, const DcPool& q, double a, double smin) { return q.v < a * p.v + smin; }

// p and the pool q above it as one pool; a = G[p.l].  The parentheses are the evaluation order.
DC_DECONV_HD DcPool dc_deconv_merge(const DcPool& p, const DcPool& q, double a) {
  const double num = p.w * p.v + (a * q.w) * q.v;
  const double den = p.w + (a * a) * q.w;
  DcPool m;
  m.v = num / den;
  m.w = den;
  m.t0 = p.t0;
  m.l = p.l + q.l;
  return m;
}

// One frame of the forward pass.  The stack holds n pools: `top` is the highest (meaningless while n == 0), the n - 1 below it lie
// in `st`, pool i at st.load(i) / st.store(i, .).  Pushes the pool (x, 1, t, 1) and merges downwards while the pool below the top
// is violated.  A pool of st is only read when it is compared and only written when a new pool comes to lie above it, so a
// frame that merges nothing stores once and loads nothing.
template <class Stack>
DC_DECONV_HD void dc_deconv_push(DcPool& top, int32_t& n, Stack& st, double x, long t, const double* G, double smin) {
  DcPool cur = dc_deconv_new(x, t);
  if (n == 0) {
    top = cur;
    n = 1;
    return;
  }
  int32_t m = n - 1;                         // the pools of st that lie below cur
  DcPool p = top;                            // the pool right below cur:
  bool held = true;                          //   the old top, which st does not hold (true), or pool m - 1 of st (false)
  bool below = true;                         // is there a pool below cur at all
  for (;;) {
    const double a = G[p.l];
    if (!dc_deconv_violates(p, cur, a, smin)) break;
    cur = dc_deconv_merge(p, cur, a);
    if (held) held = false;                  // the old top is gone
    else --m;                                // pool m - 1 of st is gone
    if (m == 0) {
      below = false;
      break;
    }
    p = st.load(m - 1);
  }
  if (below && held) st.store(m++, p);       // nothing merged: the old top becomes the highest pool of st
  top = cur;
  n = m + 1;
}

// calcium of frame t0 + k of a pool of value v: b G[k] with b = v where v > 0 and +0.0 otherwise
DC_DECONV_HD double dc_deconv_calcium(double v, double Gk) {
  const double b = v > 0.0 ? v : 0.0;
  return b * Gk;
}

// the spike at the first frame of a pool that has a pool below it: c is its own calcium there, cprev the calcium one frame earlier
DC_DECONV_HD double dc_deconv_spike(double c, double g, double cprev) { return c - g * cprev; }

// The model as the kernels, the stack views and the host drivers of csrc/deconv.hip take it -- DcAr2 of deconv_ar2_math.h gives the
// same members --: the pool type, the planes of doubles its stacks take, and the arithmetic above under one set of names.
struct DcAr1 {
  typedef DcPool Pool;
  static const int kPlanes = 2;
  double g;                                  // the decay
  const double* G;                           // G[k] = g^k, k = 0 .. T
  // the doubles of a pool, in the order of its planes: f(plane, field)
  template <class P, class F>
  DC_DECONV_HD static void words(P& p, F f) {
    f(0, p.v);
    f(1, p.w);
  }
  DC_DECONV_HD double mu(double lam, long t, long T) const { return dc_deconv_mu(lam, g, t, T); }
  DC_DECONV_HD static DcPool fresh() { return dc_deconv_new(0.0, 0); }
  template <class Stack>
  DC_DECONV_HD void push(DcPool& top, int32_t& n, Stack& st, double x, long t, double smin) const { dc_deconv_push(top, n, st, x, t, G, smin); }
  // what calc takes beside a pool's value: nothing lies below an AR(1) pool
  DC_DECONV_HD static double below(const DcPool&) { return 0.0; }
  // calcium of frame t0 + k of a pool of value val
  DC_DECONV_HD double calc(double val, double, int32_t k) const { return dc_deconv_calcium(val, G[k]); }
  // the spike at the first frame of a pool whose calcium there is c, above the pool `under`
  DC_DECONV_HD double spike(double c, const DcPool& under) const { return dc_deconv_spike(c, g, dc_deconv_calcium(under.v, G[under.l - 1])); }
};

// ---- the host restatement, over the model: the host entry points, the search of deconv_search_math.h and the stand-alone checks ----
// (host functions: no attribute)
#include <vector>

template <class Pool>
struct DcHostStack {
  std::vector<Pool>* pools;
  Pool load(int32_t i) const { return (*pools)[(size_t)i]; }
  void store(int32_t i, const Pool& p) { (*pools)[(size_t)i] = p; }
};

// the forward pass of one trace of T >= 1 frames, the baseline b taken off every frame, into pool[0 .. n), which needs T entries; -> n
template <class Model, typename In>
inline int32_t dc_forward_host(const In* y, long T, const Model& m, double lam, double smin, double b, std::vector<typename Model::Pool>& pool) {
  DcHostStack<typename Model::Pool> st = {&pool};
  typename Model::Pool top = Model::fresh();
  int32_t n = 0;
  for (long t = 0; t < T; ++t) m.push(top, n, st, dc_base_data((double)y[t], b) - m.mu(lam, t, T), t, smin);
  st.store(n - 1, top);
  return n;
}

// the AR(1) pass by its decay and table
template <typename In>
inline int32_t dc_base_forward_host(const In* y, long T, double g, const double* G, double lam, double smin, double b, std::vector<DcPool>& pool) {
  return dc_forward_host(y, T, DcAr1{g, G}, lam, smin, b, pool);
}

// Without a baseline: b = +0.0 gives the same bits, because x - (+0.0) == x for every double x under round-to-nearest, -0.0 and the
// infinities included, so (y - 0.0) - mu and y - mu are one value.
template <typename In>
inline int32_t dc_deconv_forward_host(const In* y, long T, double g, const double* G, double lam, double smin, std::vector<DcPool>& pool) {
  return dc_base_forward_host(y, T, g, G, lam, smin, 0.0, pool);
}

// the calcium of the stack pool[0 .. n) of a trace, frame by frame: c takes one double per frame
template <class Model>
inline void dc_calcium_host(const std::vector<typename Model::Pool>& pool, int32_t n, const Model& m, double* c) {
  for (int32_t i = 0; i < n; ++i) {
    const typename Model::Pool& p = pool[(size_t)i];
    for (int32_t k = 0; k < p.l; ++k) c[p.t0 + k] = m.calc(p.v, Model::below(p), k);
  }
}

// the spikes of a trace of T frames whose calcium is c: one at the first frame of every pool but the lowest
template <class Model>
inline void dc_spikes_host(const std::vector<typename Model::Pool>& pool, int32_t n, const Model& m, long T, const double* c, double* s) {
  for (long t = 0; t < T; ++t) s[t] = 0.0;
  for (int32_t i = 1; i < n; ++i) {
    const int32_t t0 = pool[(size_t)i].t0;
    s[t0] = m.spike(c[t0], pool[(size_t)i - 1]);
  }
}
