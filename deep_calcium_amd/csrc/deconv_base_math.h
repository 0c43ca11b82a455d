// The arithmetic of the baseline in the AR(1) deconvolution (include/dcunet.h, "Spikes by deconvolution", "A baseline in the
// deconvolution"): the residual with a constant b taken off the data, the gain term of a pool, the clamped Newton step on the mean
// residual, the step of the joint noise-constrained search, and the host restatement of the fit and of that search.  Plain C++ like
// deconv_search_math.h, which it builds on: the same inline functions compile for the device kernels of csrc/deconv.hip, for the
// host entry points dc_trace_deconv_ar1_fit_base_host / dc_trace_deconv_ar1_constrained_base_host and into a stand-alone host
// program (tests/native/deconv_base_check.cpp, run under the address / undefined-behaviour sanitizers).  Defined bit for bit: no
// fused multiply-add and no reassociation (the pragma below, and -ffp-contract=off for deconv.hip in _build.py).
#pragma once
#pragma clang fp contract(off)
#include "deconv_search_math.h"

#define DC_BASE_MAX_ROUNDS 64                // DC_TRACE_DECONV_BASE_MAX_ROUNDS: baseline steps of the fit

// what the thread that holds the three folds of a trace does with them (DC_TRACE_DECONV_BASE_*)
#define DC_BASE_FIT 0                        // the baseline step alone: no search state
#define DC_BASE_PASS_A 1                     // the baseline step of a search round (a finished search keeps its baseline)
#define DC_BASE_PASS_B 2                     // the search step: the bracket moves, the next parameter is written
#define DC_BASE_PASS_LAST 3                  // the search step of the last round: p*, b*, RSS(p*, b*) and the status are written

// d_t = ((double)y[t] - b) - calcium[t]; dc_base_data is deconv_math.h's, where the forward pass takes b off the data
DC_DECONV_HD double dc_base_resid(double y, double b, double c) { return dc_base_data(y, b) - c; }

// a_t at the first frame of a pool of l frames whose value is above zero; Gl = G[l].  (sum G)^2 / sum G^2 over the pool's frames,
// both sums in closed form
DC_DECONV_HD double dc_base_gain(double g, double Gl) {
  const double u = (1.0 - Gl) / (1.0 - g);
  const double q = (1.0 - Gl * Gl) / (1.0 - g * g);
  return (u * u) / q;
}

// a_t of frame t of a pool (v, t0, l): +0.0 anywhere but at the first frame of a pool above zero
DC_DECONV_HD double dc_base_gain_at(double v, long t, long t0, double g, double Gl) { return t == t0 && v > 0.0 ? dc_base_gain(g, Gl) : 0.0; }

// the clamped Newton step on phi(b) = S / T = 0
DC_DECONV_HD double dc_base_step(double b, double S, double A, long T) {
  double den = 1.0 - A / (double)T;
  if (!(den > 0.25)) den = 0.25;
  return b + (S / (double)T) / den;
}

// The joint search: the plain search's state, the baseline that is carried from round to round and the one that goes with lo.
struct DcBaseSearch {
  DcSearch s;
  double b, b_lo;
};

DC_DECONV_HD DcBaseSearch dc_base_search_begin(double sigma, long T, double b0) {
  DcBaseSearch q;
  q.s = dc_search_begin(sigma, T);
  q.b = b0;
  q.b_lo = b0;
  return q;
}

// Pass A of a round: S and A have been folded at (p, b); -> b', which is also carried.  A finished search (round 0 reached the
// noise) keeps b_0.
DC_DECONV_HD double dc_base_search_newton(DcBaseSearch& q, double S, double A, long T) {
  if (q.s.phase != DC_SEARCH_DONE) q.b = dc_base_step(q.b, S, A, T);
  return q.b;
}

// Pass B of a round (and round 0): r = RSS has been evaluated at (p, q.b); -> the parameter of the next round.  The bracket moves
// as in the plain search; where lo moves, the baseline it was evaluated with goes along.
DC_DECONV_HD double dc_base_search_step(DcBaseSearch& q, double p, double r) {
  const bool round0 = q.s.phase == DC_SEARCH_START, over = q.s.phase == DC_SEARCH_DONE;
  const double next = dc_search_step(q.s, p, r);
  if (!round0 && !over && r <= q.s.target) q.b_lo = q.b;
  return next;
}

// ---- the host restatement: the host entry points and the stand-alone check ---------------------------------------------------------
// (host functions: no attribute; the forward pass with a baseline is deconv_math.h's dc_base_forward_host)
struct DcBaseSums {
  double rss, S, A;
};

// the three folds of the stack pool[0 .. n) at the baseline b: c and a are T doubles of scratch each
template <typename In>
inline DcBaseSums dc_base_sums_host(const In* y, long T, const double* G, double b, const std::vector<DcPool>& pool, int32_t n, double* c, double* a) {
  const double g = G[1];
  dc_calcium_host(pool, n, DcAr1{g, G}, c);
  for (int32_t i = 0; i < n; ++i) {
    const DcPool& p = pool[(size_t)i];
    for (int32_t k = 0; k < p.l; ++k) a[p.t0 + k] = dc_base_gain_at(p.v, p.t0 + k, p.t0, g, G[p.l]);
  }
  DcBaseSums s;
  s.rss = dc_dyn_fold_host([&](long t) { const double d = dc_base_resid((double)y[t], b, c[t]); return d * d; }, T);
  s.S = dc_dyn_fold_host([&](long t) { return dc_base_resid((double)y[t], b, c[t]); }, T);
  s.A = dc_dyn_fold_host([&](long t) { return a[t]; }, T);
  return s;
}

// The fit of one trace at fixed parameters: `rounds` baseline steps from b0; -> b_N.  pool needs T entries, c and a T doubles.
template <typename In>
inline double dc_base_fit_host(const In* y, long T, double g, const double* G, double lam, double smin, double b0, int rounds,
                               std::vector<DcPool>& pool, double* c, double* a) {
  double b = b0;
  for (int round = 0; round < rounds; ++round) {
    const int32_t n = dc_base_forward_host(y, T, g, G, lam, smin, b, pool);
    const DcBaseSums s = dc_base_sums_host(y, T, G, b, pool, n, c, a);
    b = dc_base_step(b, s.S, s.A, T);
  }
  return b;
}

// The joint search of one trace: round 0 and `rounds` more of two passes each.  -> p*, b*, RSS(p*, b*) and the status.
template <typename In>
inline void dc_base_search_host(const In* y, long T, double g, const double* G, int which, double sigma, double other, double b0, int rounds,
                                std::vector<DcPool>& pool, double* c, double* a, double* param, double* base, double* rss, int32_t* status) {
  DcBaseSearch q = dc_base_search_begin(sigma, T, b0);
  double p = 0.0;
  auto forward = [&](double b) {
    return which == DC_SEARCH_LAM ? dc_base_forward_host(y, T, g, G, p, other, b, pool) : dc_base_forward_host(y, T, g, G, other, p, b, pool);
  };
  for (int round = 0; round <= rounds; ++round) {
    if (round > 0) {
      const int32_t n = forward(q.b);
      const DcBaseSums s = dc_base_sums_host(y, T, G, q.b, pool, n, c, a);
      dc_base_search_newton(q, s.S, s.A, T);
    }
    const int32_t n = forward(q.b);
    p = dc_base_search_step(q, p, dc_base_sums_host(y, T, G, q.b, pool, n, c, a).rss);
  }
  *param = q.s.lo;
  *base = q.b_lo;
  *rss = q.s.rss_lo;
  *status = dc_search_status(q.s);
}
