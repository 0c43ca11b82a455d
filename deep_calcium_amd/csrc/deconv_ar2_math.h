// The arithmetic of the AR(2) deconvolution (include/dcunet.h, "A rise time in the deconvolution"; csrc/deconv.hip): calcium
// c[t] = g1 c[t-1] + g2 c[t-2] + s[t] with two real roots 0 < r < d < 1, g1 = d + r, g2 = -(d * r).  The pool of the AR(1) pass
// (deconv_math.h) carries one data moment; this one carries two, A and B, and with them two pools merge in a handful of
// operations however long they are: the shift identity h[m+k] = h[m] h[k] + g2 h[m-1] h[k-1] turns the sums of the upper pool into
// sums from the lower pool's first frame.  Plain C++ like deconv_math.h, on which it builds, so the same inline functions compile
// for the device kernels, for the host entry points dc_trace_deconv_ar2_host and dc_trace_deconv_ar2_constrained_host and into a
// stand-alone host program (tests/native/deconv_ar2_check.cpp, run under the address / undefined-behaviour sanitizers).  The
// result is defined bit for bit: IEEE double operations in the order written here, the parentheses included.  No fused
// multiply-add and no reassociation anywhere: the pragma below, and -ffp-contract=off for deconv.hip in _build.py.  There is no
// host tail here: the forward pass, the outputs and the search of one trace are the templates of deconv_math.h and
// deconv_search_math.h, which take this model as they take DcAr1.
#pragma once
#pragma clang fp contract(off)
#include "deconv_search_math.h"

// A pool: `l` consecutive frames from t0 on.  v is the fitted calcium at t0 and u the calcium at t0 - 1 (the last value of the
// pool below, +0.0 for the lowest pool); A = sum_k h[k] x[t0+k] and B = sum_k h[k-1] x[t0+k] (k >= 1) are the data moments.
struct DcPool2 {
  double v, u, A, B;
  int32_t t0, l;
};

// The model: the two coefficients and the three tables of T + 1 doubles each.  h[0] = 1, h[1] = g1, h[k] = g1 h[k-1] + g2 h[k-2]:
// the response to one spike.  HH[l] = sum_{k<l} h[k] h[k] and HP[l] = sum_{1<=k<l} h[k] h[k-1], by running sums from +0.0.  Its
// members are those of DcAr1 (deconv_math.h), the names under which csrc/deconv.hip and the host drivers reach the functions below.
struct DcAr2 {
  typedef DcPool2 Pool;
  static const int kPlanes = 4;
  double g1, g2;
  const double *h, *HH, *HP;
  template <class P, class F>
  DC_DECONV_HD static void words(P& p, F f) {
    f(0, p.v);
    f(1, p.u);
    f(2, p.A);
    f(3, p.B);
  }
  DC_DECONV_HD static double below(const DcPool2& p) { return p.u; }
  DC_DECONV_HD double mu(double lam, long t, long T) const;
  DC_DECONV_HD static DcPool2 fresh();
  template <class Stack>
  DC_DECONV_HD void push(DcPool2& top, int32_t& n, Stack& st, double x, long t, double smin) const;
  DC_DECONV_HD double calc(double val, double below, int32_t k) const;
  DC_DECONV_HD double spike(double c, const DcPool2& under) const;
};

// the rows of a (3, ldH) table as the entry points take it
DC_DECONV_HD DcAr2 dc_ar2_model(double g1, double g2, const double* H, long ldH) {
  DcAr2 m;
  m.g1 = g1;
  m.g2 = g2;
  m.h = H;
  m.HH = H + ldH;
  m.HP = H + 2 * ldH;
  return m;
}

// two real roots inside (0, 1), not equal; a NaN fails
DC_DECONV_HD bool dc_ar2_roots_ok(double g1, double g2) { return g2 < 0.0 && g1 > 0.0 && g1 + g2 < 1.0 && g1 * g1 + 4.0 * g2 > 0.0; }

// what is subtracted from frame t of a trace of T frames: the L1 penalty lam on the spikes, written as a shift of the data
DC_DECONV_HD double dc_ar2_mu(double lam, double g1, double g2, long t, long T) {
  if (t < T - 2) return lam * ((1.0 - g1) - g2);
  if (t == T - 2) return lam * (1.0 - g1);
  return lam;
}

// calcium of frame t0 + k of a pool of value v above the calcium u
DC_DECONV_HD double dc_ar2_calc(const DcAr2& m, double v, double u, int32_t k) {
  const double b = v > 0.0 ? v : 0.0;
  if (k == 0) return b;
  return m.h[k] * b + (m.g2 * m.h[k - 1]) * u;
}

// the least-squares value of a pool of l frames and moment A, given u
DC_DECONV_HD double dc_ar2_fit(const DcAr2& m, double A, double u, int32_t l) { return (A - (m.g2 * u) * m.HP[l]) / m.HH[l]; }

// What a comparison with the pool of l frames below, and the merge with it, take from the table: h[l], h[l-1], h[l-2], h[l-3].  All
// four are loaded at once and without a branch -- an index below zero is read at 0 and its value not used --, so a lane waits for
// one round trip to the table and not for one per branch: the forward pass is bound by that latency.
struct DcAr2Taps {
  double h0, h1, h2, h3;
};
DC_DECONV_HD DcAr2Taps dc_ar2_taps(const DcAr2& m, int32_t l) {
  DcAr2Taps t;
  t.h0 = m.h[l];
  t.h1 = m.h[l - 1];
  t.h2 = m.h[l >= 2 ? l - 2 : 0];
  t.h3 = m.h[l >= 3 ? l - 3 : 0];
  return t;
}

// the last two values of pool p, as the pool above it sees them: calc(p, l - 1), and calc(p, l - 2) or, for l = 1, u
DC_DECONV_HD void dc_ar2_tail(const DcAr2& m, const DcPool2& p, const DcAr2Taps& t, double& last, double& sec) {
  const double b = p.v > 0.0 ? p.v : 0.0;
  const double far = t.h2 * b + (m.g2 * t.h3) * p.u;
  last = p.l == 1 ? b : t.h1 * b + (m.g2 * t.h2) * p.u;
  sec = p.l == 1 ? p.u : p.l == 2 ? b : far;
}
DC_DECONV_HD void dc_ar2_tail(const DcAr2& m, const DcPool2& p, double& last, double& sec) { dc_ar2_tail(m, p, dc_ar2_taps(m, p.l), last, sec); }

// does a pool of value v start below what the pool under it continues to, plus the smallest spike allowed?
DC_DECONV_HD bool dc_ar2_violates(const DcAr2& m, double v, double last, double sec, double smin) {
  return v < (m.g1 * last + m.g2 * sec) + smin;
}

// the spike at the first frame of a pool that has a pool below it: c is its own calcium there
DC_DECONV_HD double dc_ar2_spike(const DcAr2& m, double c, double last, double sec) { return (c - m.g1 * last) - m.g2 * sec; }

DC_DECONV_HD DcPool2 dc_ar2_new(double x, long t) {
  DcPool2 q;
  q.v = 0.0;                                 // fitted once u is known
  q.u = 0.0;
  q.A = x;
  q.B = 0.0;
  q.t0 = (int32_t)t;
  q.l = 1;
  return q;
}

// p and the pool q above it as one pool: the moments only, u and v are the caller's.  t = dc_ar2_taps(m, p.l).  The parentheses
// are the evaluation order.
DC_DECONV_HD DcPool2 dc_ar2_merge(const DcAr2& m, const DcPool2& p, const DcPool2& q, const DcAr2Taps& t) {
  const double h2 = p.l >= 2 ? t.h2 : 0.0;
  DcPool2 r;
  r.v = 0.0;
  r.u = 0.0;
  r.A = (p.A + t.h0 * q.A) + (m.g2 * t.h1) * q.B;
  r.B = (p.B + t.h1 * q.A) + (m.g2 * h2) * q.B;
  r.t0 = p.t0;
  r.l = p.l + q.l;
  return r;
}

// One frame of the forward pass, in the shape of dc_deconv_push: the stack holds n pools, `top` the highest (meaningless while
// n == 0), the n - 1 below it in `st`.  Pushes the pool of frame t and merges downwards while the pool below it is violated; the
// pool that ends on top is fitted against the pool below it, or against +0.0 where there is none.  A pool of st is only read when
// it is compared and only written when a new pool comes to lie above it.
template <class Stack>
DC_DECONV_HD void dc_ar2_push(DcPool2& top, int32_t& n, Stack& st, double x, long t, const DcAr2& m, double smin) {
  DcPool2 cur = dc_ar2_new(x, t);
  int32_t k = n - 1;                         // the pools of st that lie below cur
  DcPool2 p = top;                           // the pool right below cur:
  bool held = true;                          //   the old top, which st does not hold (true), or pool k - 1 of st (false)
  bool below = n > 0;                        // is there a pool below cur at all
  while (below) {
    const DcAr2Taps taps = dc_ar2_taps(m, p.l);
    double last, sec;
    dc_ar2_tail(m, p, taps, last, sec);
    cur.u = last;
    cur.v = dc_ar2_fit(m, cur.A, cur.u, cur.l);
    if (!dc_ar2_violates(m, cur.v, last, sec, smin)) break;
    cur = dc_ar2_merge(m, p, cur, taps);
    if (held) held = false;                  // the old top is gone
    else --k;                                // pool k - 1 of st is gone
    if (k == 0) below = false;
    else p = st.load(k - 1);
  }
  if (!below) {
    k = 0;
    cur.u = 0.0;
    cur.v = dc_ar2_fit(m, cur.A, cur.u, cur.l);
  } else if (held) {
    st.store(k++, p);                        // nothing merged: the old top becomes the highest pool of st
  }
  top = cur;
  n = k + 1;
}

// ---- the members of the model: the functions above under the names of DcAr1 ---------------------------------------------------------
DC_DECONV_HD double DcAr2::mu(double lam, long t, long T) const { return dc_ar2_mu(lam, g1, g2, t, T); }
DC_DECONV_HD DcPool2 DcAr2::fresh() { return dc_ar2_new(0.0, 0); }
template <class Stack>
DC_DECONV_HD void DcAr2::push(DcPool2& top, int32_t& n, Stack& st, double x, long t, double smin) const { dc_ar2_push(top, n, st, x, t, *this, smin); }
DC_DECONV_HD double DcAr2::calc(double val, double below, int32_t k) const { return dc_ar2_calc(*this, val, below, k); }
DC_DECONV_HD double DcAr2::spike(double c, const DcPool2& under) const {
  double last, sec;
  dc_ar2_tail(*this, under, last, sec);
  return dc_ar2_spike(*this, c, last, sec);
}
