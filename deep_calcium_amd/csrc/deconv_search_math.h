// The arithmetic of the noise-constrained search (include/dcunet.h, "Spikes by deconvolution", dc_trace_deconv_ar1_constrained): the
// residual term, the step that moves one trace's bracket, and the host restatement of the whole search.  Plain C++ like
// deconv_math.h, which it builds on: the same inline functions compile for the device kernels of csrc/deconv.hip, for the host entry
// point dc_trace_deconv_ar1_constrained_host and into a stand-alone host program (tests/native/deconv_search_check.cpp, run under
// the address / undefined-behaviour sanitizers).  There is one search: the step never sees the model, and the host loop is a
// template over it (DcAr1 here, DcAr2 of deconv_ar2_math.h), as the sweep kernel is.  The host forward pass is deconv_math.h's,
// the fold of the residual the one of trace_dyn_math.h.  Defined bit for bit: no fused multiply-add and no reassociation (the pragma below, and -ffp-contract=off for
// deconv.hip in _build.py).
#pragma once
#pragma clang fp contract(off)
#include "deconv_math.h"
#include "trace_dyn_math.h"

#define DC_SEARCH_SMIN 0                     // DC_TRACE_DECONV_SEARCH_SMIN: `which`
#define DC_SEARCH_LAM 1                      // DC_TRACE_DECONV_SEARCH_LAM
#define DC_SEARCH_MAX_ROUNDS 64              // DC_TRACE_DECONV_SEARCH_MAX_ROUNDS

// what a trace's search is doing
#define DC_SEARCH_START 0                    // round 0 (p = 0) is being evaluated
#define DC_SEARCH_EXPAND 1                   // hi has never failed: it doubles
#define DC_SEARCH_BISECT 2                   // RSS(hi) > target: the bracket halves
#define DC_SEARCH_DONE 3                     // RSS(0) >= target: p* = 0

struct DcSearch {
  double lo, hi, rss_lo, target;
  int32_t phase;
};

// one term of the residual fold: the product is rounded once
DC_DECONV_HD double dc_search_term(double y, double c) {
  const double d = y - c;
  return d * d;
}

DC_DECONV_HD double dc_search_target(double sigma, long T) { return (sigma * sigma) * (double)T; }

// before round 0; the parameter of round 0 is 0.0
DC_DECONV_HD DcSearch dc_search_begin(double sigma, long T) {
  DcSearch s;
  s.lo = 0.0;
  s.hi = sigma;
  s.rss_lo = 0.0;
  s.target = dc_search_target(sigma, T);
  s.phase = DC_SEARCH_START;
  return s;
}

// One round: r = RSS(p) has been evaluated; -> the parameter of the next round.
DC_DECONV_HD double dc_search_step(DcSearch& s, double p, double r) {
  if (s.phase == DC_SEARCH_START) {
    s.rss_lo = r;
    if (!(r < s.target)) {                   // the unconstrained residual already reaches the noise: finished
      s.phase = DC_SEARCH_DONE;
      return 0.0;
    }
    s.phase = DC_SEARCH_EXPAND;
    return s.hi;
  }
  if (s.phase == DC_SEARCH_DONE) return 0.0;
  if (r <= s.target) {
    s.lo = p;
    s.rss_lo = r;
    if (s.phase == DC_SEARCH_EXPAND) s.hi = s.hi + s.hi;
  } else {
    s.hi = p;
    s.phase = DC_SEARCH_BISECT;
  }
  return s.phase == DC_SEARCH_EXPAND ? s.hi : 0.5 * (s.lo + s.hi);
}

// 0: bracketed; 1: p* = 0, the residual reaches the noise unconstrained; 2: never bracketed, the constraint is still slack at p*
DC_DECONV_HD int32_t dc_search_status(const DcSearch& s) { return s.phase == DC_SEARCH_DONE ? 1 : s.phase == DC_SEARCH_EXPAND ? 2 : 0; }

// ---- the host restatement, over the model (DcAr1, DcAr2): the *_constrained_host entry points and the stand-alone checks ----------
// (host functions: no attribute)
// RSS of the stack pool[0 .. n): c is T doubles of scratch
template <class Model, typename In>
inline double dc_rss_host(const In* y, long T, const Model& m, const std::vector<typename Model::Pool>& pool, int32_t n, double* c) {
  dc_calcium_host(pool, n, m, c);
  return dc_dyn_fold_host([&](long t) { return dc_search_term((double)y[t], c[t]); }, T);
}

// The search of one trace: round 0 and `rounds` more.  -> p*, RSS(p*) and the status; pool needs T entries, c T doubles.
template <class Model, typename In>
inline void dc_search_host(const In* y, long T, const Model& m, int which, double sigma, double other, int rounds,
                           std::vector<typename Model::Pool>& pool, double* c, double* param, double* rss, int32_t* status) {
  DcSearch s = dc_search_begin(sigma, T);
  double p = 0.0;
  for (int round = 0; round <= rounds; ++round) {
    const int32_t n = which == DC_SEARCH_LAM ? dc_forward_host(y, T, m, p, other, 0.0, pool) : dc_forward_host(y, T, m, other, p, 0.0, pool);
    p = dc_search_step(s, p, dc_rss_host(y, T, m, pool, n, c));
  }
  *param = s.lo;
  *rss = s.rss_lo;
  *status = dc_search_status(s);
}
