// The arithmetic of the trace dynamics (include/dcunet.h, "Trace dynamics: noise and AR(1) decay"; csrc/trace_dyn.hip): the robust
// noise of a trace from its first difference, the fixed-order fold, the autocovariance, the least-squares decay and the
// least-squares AR(2) coefficients ("Trace dynamics: AR(2) coefficients"; tests/native/trace_dyn_ar2_check.cpp).  Plain C++
// like deconv_math.h, so the same inline functions compile for the device kernels, for the host entry point
// dc_trace_ar1_estimate_host and into a stand-alone host program (tests/native/trace_dyn_math_check.cpp, run under the address /
// undefined-behaviour sanitizers).  The results are defined bit for bit: the noise by VALUE (medians: any selection algorithm gives
// the same number), everything else by IEEE double operations in the order written here.  No fused multiply-add and no
// reassociation anywhere: the pragma below, and -ffp-contract=off for trace_dyn.hip in _build.py.
#pragma once
#pragma clang fp contract(off)
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DC_DYN_HD __host__ __device__ inline
#else
#define DC_DYN_HD inline
#endif

#define DC_DYN_LANES 256                     // DC_TRACE_DYN_LANES: the width of the fold
#define DC_DYN_MAX_LAGS 16                   // DC_TRACE_DYN_MAX_LAGS

// ---- the noise: medians by value --------------------------------------------------------------------------------------------------
// A 64-bit key that orders doubles as numbers (-0.0 just below +0.0; NaN is never fed): the selection counts keys, not values.
DC_DYN_HD uint64_t dc_dyn_key(double x) {
  uint64_t u;
  memcpy(&u, &x, 8);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
DC_DYN_HD double dc_dyn_unkey(uint64_t k) {
  const uint64_t u = (k >> 63) ? (k ^ 0x8000000000000000ull) : ~k;
  double x;
  memcpy(&x, &u, 8);
  return x;
}
// the value the first median ranks (dev = false: d[t] = y[t+1] - y[t]) and the one the second ranks (dev = true: |d[t] - m|)
DC_DYN_HD double dc_dyn_value(double y0, double y1, bool dev, double m) {
  const double d = y1 - y0;
  return dev ? fabs(d - m) : d;
}
// the median of an even number of values from its two middle ones, as numpy forms it
DC_DYN_HD double dc_dyn_mid(double lo, double hi) { return (lo + hi) / 2.0; }
// sigma from the median absolute deviation: (1.4826 * mad) / sqrt(2.0), the square root being the correctly rounded constant
DC_DYN_HD double dc_dyn_sigma(double mad) { return (1.4826 * mad) / 0x1.6a09e667f3bcdp+0; }

// ---- the decay -----------------------------------------------------------------------------------------------------------------------
// one term of an autocovariance fold: both factors are centred first, the product is rounded once
DC_DYN_HD double dc_dyn_term(double a, double b, double mean) { return (a - mean) * (b - mean); }

// g_raw from xc[0 .. lags]: least squares of xc[i+1] on A[i], A[0] = xc[0] - sn * sn, A[i] = xc[i]; left folds from +0.0 over
// ascending i.  NaN where the estimate is undefined: T < lags + 2, a zero denominator, a quotient that is not finite.
DC_DYN_HD double dc_dyn_decay(const double* xc, int lags, double sn, long T) {
  double num = 0.0, den = 0.0;
  for (int i = 0; i < lags; ++i) {
    const double A = i == 0 ? xc[0] - sn * sn : xc[i];
    num = num + A * xc[i + 1];
    den = den + A * A;
  }
  if (T < (long)lags + 2 || den == 0.0) return NAN;
  const double q = num / den;
  return isfinite(q) ? q : NAN;
}

// (g1_raw, g2_raw) from xc[0 .. lags], lags >= 2: least squares of y_i = xc[i+1] on the two columns a and b of
// toeplitz(xc[0 .. lags-1], xc[0 .. 1]) - sn^2 I, rows i = 0 .. lags-1; the five sums are left folds from +0.0 over ascending i,
// the 2 x 2 system is solved by its determinant.  No roots are taken here.  Both NaN where the estimate is undefined:
// T < lags + 2, a determinant that is not positive (NaN included), a quotient that is not finite.
DC_DYN_HD void dc_dyn_ar2_solve(const double* xc, int lags, double sn, long T, double* g1_raw, double* g2_raw) {
  const double c0 = xc[0] - sn * sn;
  double Saa = 0.0, Sab = 0.0, Sbb = 0.0, Say = 0.0, Sby = 0.0;
  for (int i = 0; i < lags; ++i) {
    const double a = i == 0 ? c0 : xc[i];
    const double b = i == 0 ? xc[1] : i == 1 ? c0 : xc[i - 1];
    const double y = xc[i + 1];
    Saa = Saa + a * a;
    Sab = Sab + a * b;
    Sbb = Sbb + b * b;
    Say = Say + a * y;
    Sby = Sby + b * y;
  }
  const double det = Saa * Sbb - Sab * Sab;
  *g1_raw = *g2_raw = NAN;
  if (T < (long)lags + 2 || !(det > 0.0)) return;
  const double g1 = (Say * Sbb - Sby * Sab) / det;
  const double g2 = (Saa * Sby - Sab * Say) / det;
  if (!isfinite(g1) || !isfinite(g2)) return;
  *g1_raw = g1;
  *g2_raw = g2;
}

// ---- the host restatement: dc_trace_ar1_estimate_host and the stand-alone check ---------------------------------------------------
// (host functions: no attribute)
#include <algorithm>
#include <vector>

// fold(f, n): 256 lane sums over t = j, j + 256, ... ascending, from +0.0; then the tree h = 128 .. 1, P[j] = P[j] + P[j + h].
// On the device (trace_dyn.hip, deconv.hip) thread j of a 256-thread workgroup forms lane sum j and dc_dyn_fold_tree is the tree:
// `rows` folds at once, the lane sums of fold l at red[l * 256 + j] in LDS, its result at red[l * 256]; a barrier before every
// step and one after the last.
#if defined(__HIPCC__)
__device__ __forceinline__ void dc_dyn_fold_tree(double* red, int rows) {
  const int tid = threadIdx.x;
  for (int h = DC_DYN_LANES / 2; h >= 1; h >>= 1) {
    __syncthreads();
    if (tid < h)
      for (int l = 0; l < rows; ++l) red[l * DC_DYN_LANES + tid] = red[l * DC_DYN_LANES + tid] + red[l * DC_DYN_LANES + tid + h];
  }
  __syncthreads();
}
#endif
template <class F>
inline double dc_dyn_fold_host(F f, long n) {
  double P[DC_DYN_LANES];
  for (int j = 0; j < DC_DYN_LANES; ++j) {
    double s = 0.0;
    for (long t = j; t < n; t += DC_DYN_LANES) s = s + f(t);
    P[j] = s;
  }
  for (int h = DC_DYN_LANES / 2; h >= 1; h >>= 1)
    for (int j = 0; j < h; ++j) P[j] = P[j] + P[j + h];
  return P[0];
}

// med(x) of n >= 1 values (x is reordered): the (n-1)/2-th smallest for odd n, the mean of the two middle ones for even n
inline double dc_dyn_median_host(std::vector<double>& x) {
  const size_t n = x.size(), k = n / 2;
  std::nth_element(x.begin(), x.begin() + (long)k, x.end());
  const double hi = x[k];
  if (n & 1) return hi;
  return dc_dyn_mid(*std::max_element(x.begin(), x.begin() + (long)k), hi);
}

template <typename In>
inline double dc_dyn_noise_host(const In* y, long T, std::vector<double>& x) {
  if (T < 3) return 0.0;
  x.resize((size_t)(T - 1));
  for (long t = 0; t < T - 1; ++t) x[(size_t)t] = dc_dyn_value((double)y[t], (double)y[t + 1], false, 0.0);
  const double m = dc_dyn_median_host(x);
  for (long t = 0; t < T - 1; ++t) x[(size_t)t] = dc_dyn_value((double)y[t], (double)y[t + 1], true, m);
  return dc_dyn_sigma(dc_dyn_median_host(x));
}

// xc[0 .. lags] of one trace of T >= 1 frames
template <typename In>
inline void dc_dyn_autocov_host(const In* y, long T, int lags, double* xc) {
  const double mean = dc_dyn_fold_host([&](long t) { return (double)y[t]; }, T) / (double)T;
  for (int l = 0; l <= lags; ++l)
    xc[l] = dc_dyn_fold_host([&](long t) { return dc_dyn_term((double)y[t], (double)y[t + l], mean); }, T - l) / (double)T;
}
