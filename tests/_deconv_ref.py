"""The oracle of the AR(1) deconvolution (include/dcunet.h, "Spikes by deconvolution"): the forward pass and the outputs in plain
Python floats -- IEEE doubles, one rounding per operation, evaluated in the order the header writes them --, an independent
cross-check in exact rationals, the generator and the matching rule of the reach table, and the ctypes call of the library's
host entry point that the CPU and the GPU tests share."""
import ctypes
import itertools
from fractions import Fraction

import numpy as np


def table(g, T):
    G = [1.0]
    for _ in range(T):
        G.append(G[-1] * g)
    return G


def forward(y, G, lam, smin):
    """-> the final stack of pools [v, w, t0, l] of one trace."""
    T = len(y)
    g = G[1]
    pools = []
    for t in range(T):
        mu = lam * (1.0 - g) if t < T - 1 else lam
        pools.append([float(y[t]) - mu, 1.0, t, 1])
        while len(pools) >= 2 and pools[-1][0] < G[pools[-2][3]] * pools[-2][0] + smin:
            q = pools.pop()
            p = pools[-1]
            a = G[p[3]]
            num = p[1] * p[0] + (a * q[1]) * q[0]
            den = p[1] + (a * a) * q[1]
            p[0] = num / den
            p[1] = den
            p[3] += q[3]
    return pools


def outputs(pools, G, T):
    g = G[1]
    c, s = [0.0] * T, [0.0] * T
    for i, (v, _, t0, l) in enumerate(pools):
        b = v if v > 0.0 else 0.0
        for k in range(l):
            c[t0 + k] = b * G[k]
        if i >= 1:
            s[t0] = c[t0] - g * c[t0 - 1]
    return c, s


def deconvolve(y, g, lam=0.0, smin=0.0):
    """(R, T) float32 / float64 -> calcium float64 (R, T), spikes float64 (R, T), pools int32[R]."""
    y = np.asarray(y)
    R, T = y.shape
    lam = np.broadcast_to(np.asarray(lam, np.float64), (R,))
    smin = np.broadcast_to(np.asarray(smin, np.float64), (R,))
    G = table(float(g), T)
    c, s, n = np.empty((R, T)), np.empty((R, T)), np.empty(R, np.int32)
    for r in range(R):
        pools = forward(y[r], G, float(lam[r]), float(smin[r]))
        c[r], s[r] = outputs(pools, G, T)
        n[r] = len(pools)
    return c, s, n


def same_bits(a, b):
    """Equal in every bit: the sign of a zero counts."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- exact rationals -------------------------------------------------------------------------------------------------------------
def forward_exact(y, g, lam):
    """The same forward pass (smin = 0) in Fractions: no rounding anywhere."""
    T = len(y)
    pools = []
    for t in range(T):
        mu = lam * (1 - g) if t < T - 1 else lam
        pools.append([Fraction(y[t]) - mu, Fraction(1), t, 1])
        while len(pools) >= 2 and pools[-1][0] < g ** pools[-2][3] * pools[-2][0]:
            q = pools.pop()
            p = pools[-1]
            a = g ** p[3]
            p[0], p[1] = (p[1] * p[0] + a * q[1] * q[0]) / (p[1] + a * a * q[1]), p[1] + a * a * q[1]
            p[3] += q[3]
    return pools


def solve_exact(y, g, lam):
    """Independent of any pool algorithm: the minimiser of 1/2 sum (c_t - y_t)^2 + lam (c_0 + sum_{t>=1} (c_t - g c_{t-1})) subject
    to c_t >= g c_{t-1}, by enumeration.  The penalty is linear in c: it moves the data to x_t = y_t - mu_t.  Within a run of
    tight constraints c is v g^k and the best v is the least-squares one; of the 2^(T-1) ways to cut the trace into runs the
    feasible ones (every cut a spike >= 0) contain the optimum of this convex problem, so the feasible cut of least cost is it."""
    T = len(y)
    x = [Fraction(y[t]) - (lam * (1 - g) if t < T - 1 else lam) for t in range(T)]
    best = None
    for cuts in itertools.product((0, 1), repeat=T - 1):
        starts = [0] + [t + 1 for t in range(T - 1) if cuts[t]]
        c = []
        for i, t0 in enumerate(starts):
            l = (starts[i + 1] if i + 1 < len(starts) else T) - t0
            v = sum(g ** k * x[t0 + k] for k in range(l)) / sum(g ** (2 * k) for k in range(l))
            c += [v * g ** k for k in range(l)]
        if all(c[t] >= g * c[t - 1] for t in starts[1:]):
            cost = sum((a - b) ** 2 for a, b in zip(c, x))
            if best is None or cost < best[0]:
                best = (cost, c)
    return best[1]


# ---- the reach table ---------------------------------------------------------------------------------------------------------------
def reach_trace(seed, sigma, T=1024):
    rs = np.random.RandomState(seed)
    sp = (rs.poisson(0.03, T) > 0)
    c0 = np.convolve(sp, np.exp(-np.arange(T) / 8.0))[:T]
    y = np.float32(c0 + sigma * rs.standard_normal(T))
    return sp, y


def match(true_frames, event_frames, tol=2):
    """The true spikes in time order; each takes the nearest unused event within +-tol frames, the earlier one on a tie."""
    used, hits = set(), 0
    events = sorted(int(e) for e in event_frames)
    for t in sorted(int(x) for x in true_frames):
        near = [(abs(e - t), e) for e in events if abs(e - t) <= tol and e not in used]
        if near:
            used.add(min(near)[1])
            hits += 1
    return hits


def prf(hits, n_true, n_events):
    rec = hits / n_true if n_true else 1.0
    pre = hits / n_events if n_events else 1.0
    return rec, pre, (2 * rec * pre / (rec + pre) if rec + pre else 0.0)


# ---- the library's host entry point ----------------------------------------------------------------------------------------------
def host_entry(L, y, g, lam=0.0, smin=0.0, pad=0):
    """dc_trace_deconv_ar1_host on the rows of y, stored with stride T + pad (the padding holds NaN: it must not be read into a
    result), outputs pre-filled with NaN.  -> calcium, spikes, pools."""
    from deep_calcium_amd.deconv import ar1_table
    y = np.asarray(y)
    R, T = y.shape
    buf = np.full((R, T + pad), np.nan, y.dtype)
    buf[:, :T] = y
    G = ar1_table(g, T)
    lam = np.broadcast_to(np.asarray(lam, np.float64), (R,)).copy()
    smin = np.broadcast_to(np.asarray(smin, np.float64), (R,)).copy()
    c, s, n = np.full((R, T), np.nan), np.full((R, T), np.nan), np.full(R, -1, np.int32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                  # noqa: E731
    L.dc_trace_deconv_ar1_host(ptr(buf), int(y.dtype == np.float64), T + pad, R, T, ptr(G), ptr(lam), ptr(smin), ptr(c), ptr(s), ptr(n))
    return c, s, n
