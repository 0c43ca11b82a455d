"""The oracle of the trace dynamics (include/dcunet.h, "Trace dynamics: noise and AR(1) decay"): the noise is numpy's trace_noise
(medians are values: any selection gives the same number); the fold, the autocovariance and the decay are plain Python floats --
IEEE doubles, one rounding per operation, evaluated in the order the header writes them --, with an independent check of every
folded sum against math.fsum, and the ctypes call of the library's host entry point that the CPU and the GPU tests share."""
import ctypes
import math

import numpy as np

W = 256                               # DC_TRACE_DYN_LANES


def noise(y):
    from deep_calcium_amd.deconv import trace_noise
    return trace_noise(np.asarray(y))


def fold(terms):
    """terms: the values f(0), f(1), ..., f(n-1) as Python floats."""
    n = len(terms)
    P = [0.0] * W
    for j in range(min(W, n)):
        s = 0.0
        for t in range(j, n, W):
            s = s + terms[t]
        P[j] = s
    h = W // 2
    while h >= 1:
        for j in range(h):
            P[j] = P[j] + P[j + h]
        h //= 2
    return P[0]


def fold_bound(terms):
    """The rounding bound of fold() against the exact sum: a term passes through at most ceil(n / 256) additions in its lane
    (the first, to +0.0, is exact) and 8 in the tree; every addition rounds a partial sum that is at most sum |term| (1 + small)
    in magnitude by at most 2^-53 of it.  (ceil(n / 256) + 9) 2^-53 sum |term| carries one unit for the second-order terms."""
    n = len(terms)
    return (math.ceil(n / W) + 9) * 2.0 ** -53 * math.fsum(abs(v) for v in terms)


def autocov_terms(y, lags):
    """-> (mean, [terms of q_0, ..., terms of q_lags]) of one trace: what the folds sum, each term rounded as the header says."""
    y = [float(v) for v in y]
    T = len(y)
    mean = fold(y) / float(T)
    c = [v - mean for v in y]
    return mean, [[c[t] * c[t + l] for t in range(max(T - l, 0))] for l in range(lags + 1)]


def autocov(y, lags):
    T = len(y)
    _, terms = autocov_terms(y, lags)
    return [fold(q) / float(T) for q in terms]


def decay(xc, lags, sn, T):
    num = den = 0.0
    for i in range(lags):
        A = xc[0] - sn * sn if i == 0 else xc[i]
        num = num + A * xc[i + 1]
        den = den + A * A
    if T < lags + 2 or den == 0.0:
        return math.nan
    q = num / den
    return q if math.isfinite(q) else math.nan


def estimate(y, lags=5, sn=None):
    """(R, T) float32 / float64 -> sigma float64[R], xc float64 (R, lags + 1), g_raw float64[R]."""
    y = np.asarray(y)
    R, T = y.shape
    sigma = noise(y)
    xc = np.empty((R, lags + 1))
    g = np.empty(R)
    for r in range(R):
        xc[r] = autocov(y[r], lags)
        g[r] = decay([float(v) for v in xc[r]], lags, float(sigma[r] if sn is None else np.broadcast_to(sn, (R,))[r]), T)
    return sigma, xc, g


def same_bits(a, b):
    """Equal in every bit: the sign of a zero counts, and so does the NaN (the library's undefined g_raw is C's NAN, the oracle's
    is math.nan: both the positive quiet NaN with an empty payload)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def traces(R, T, seed, dtype=np.float32):
    """Rows in turn: events of decay 8 frames on noise, pure noise, a drifting trace with large values, values quantised to 8
    levels (the selection meets many ties), an all-negative trace, a noise-free exponential."""
    rs = np.random.RandomState(seed)
    t = np.arange(T)
    y = np.empty((R, T))
    for r in range(R):
        kind = r % 6
        if kind == 0:
            sp = rs.poisson(0.05, T) > 0
            y[r] = np.convolve(sp, np.exp(-t / 8.0))[:T] + 0.2 * rs.standard_normal(T)
        elif kind == 1:
            y[r] = 0.5 * rs.standard_normal(T)
        elif kind == 2:
            y[r] = 100.0 * np.cumsum(rs.standard_normal(T)) / np.sqrt(T) + 3.0
        elif kind == 3:
            y[r] = rs.randint(0, 8, T) / 4.0 - 1.0
        elif kind == 4:
            y[r] = -5.0 - np.abs(rs.standard_normal(T))
        else:
            y[r] = 3.0 * 0.9 ** t
    return y.astype(dtype)


# ---- the library's host entry point ----------------------------------------------------------------------------------------------
def host_entry(L, y, lags=5, sn=None, pad=0, want_sigma=True):
    """dc_trace_ar1_estimate_host on the rows of y, stored with stride T + pad (the padding holds NaN: it must not be read into a
    result), outputs pre-filled with NaN.  -> sigma, xc, g_raw."""
    y = np.asarray(y)
    R, T = y.shape
    buf = np.full((R, T + pad), np.nan, y.dtype)
    buf[:, :T] = y
    sigma, xc, g = np.full(R, np.nan), np.full((R, lags + 1), np.nan), np.full(R, -7.0)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                  # noqa: E731
    snb = None if sn is None else np.broadcast_to(np.asarray(sn, np.float64), (R,)).copy()
    L.dc_trace_ar1_estimate_host(ptr(buf), int(y.dtype == np.float64), T + pad, R, T, lags, None if snb is None else ptr(snb),
                                 ptr(sigma) if want_sigma else None, ptr(xc), ptr(g))
    return sigma, xc, g
