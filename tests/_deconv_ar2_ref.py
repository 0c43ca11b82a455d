"""The oracle of the AR(2) deconvolution (include/dcunet.h, "A rise time in the deconvolution"): the tables, the forward pass, the
outputs and the residual of the noise-constrained search in plain Python floats -- IEEE doubles, one rounding per operation,
evaluated in the order the header writes them --, the same pass in exact rationals, the generator of the reach table, and the
ctypes calls of the library's host entry points that the CPU and the GPU tests share.  The search itself is
_deconv_search_ref's: only RSS(p) differs."""
import ctypes
import math
from fractions import Fraction

import numpy as np

import _deconv_ref as ref
import _deconv_search_ref as sr

ROOTS = ((0.75, 0.25), (math.exp(-1.0 / 8), math.exp(-1.0 / 2)), (0.99, 0.9), (0.5, 0.01))     # (d, r)


def coefficients(d, r):
    return d + r, -(d * r)


def table(d, r, T):
    """-> h, HH, HP: lists of T + 1 floats."""
    g1, g2 = coefficients(d, r)
    h = [1.0, g1]
    for k in range(2, T + 1):
        h.append(g1 * h[k - 1] + g2 * h[k - 2])
    h = h[:T + 1]
    HH, HP = [0.0], [0.0]
    for l in range(T):
        HH.append(HH[l] + h[l] * h[l])
        HP.append(HP[l] + (h[l] * h[l - 1] if l >= 1 else 0.0))
    return h, HH, HP


class Model(object):
    def __init__(self, d, r, T):
        self.d, self.r, self.T = float(d), float(r), T
        self.g1, self.g2 = coefficients(self.d, self.r)
        self.h, self.HH, self.HP = table(self.d, self.r, T)

    def calc(self, v, u, k):
        b = v if v > 0.0 else 0.0
        if k == 0:
            return b
        return self.h[k] * b + (self.g2 * self.h[k - 1]) * u

    def fit(self, A, u, l):
        return (A - (self.g2 * u) * self.HP[l]) / self.HH[l]

    def tail(self, p):
        """last, sec of the pool p = [v, u, A, B, t0, l]"""
        v, u, _, _, _, l = p
        return self.calc(v, u, l - 1), (self.calc(v, u, l - 2) if l >= 2 else u)

    def mu(self, lam, t):
        T = self.T
        if t < T - 2:
            return lam * ((1.0 - self.g1) - self.g2)
        if t == T - 2:
            return lam * (1.0 - self.g1)
        return lam


def forward(y, m, lam, smin, base=0.0):
    """-> the final stack of pools [v, u, A, B, t0, l] of one trace."""
    h, g1, g2 = m.h, m.g1, m.g2
    pools = []
    for t in range(len(y)):
        x = (float(y[t]) - base) - m.mu(lam, t)
        cur = [0.0, 0.0, x, 0.0, t, 1]
        while True:
            if not pools:
                cur[1] = 0.0
                cur[0] = m.fit(cur[2], 0.0, cur[5])
                break
            p = pools[-1]
            last, sec = m.tail(p)
            cur[1] = last
            cur[0] = m.fit(cur[2], last, cur[5])
            if not cur[0] < (g1 * last + g2 * sec) + smin:
                break
            n = p[5]
            A = (p[2] + h[n] * cur[2]) + (g2 * h[n - 1]) * cur[3]
            B = (p[3] + h[n - 1] * cur[2]) + (g2 * (h[n - 2] if n >= 2 else 0.0)) * cur[3]
            cur = [0.0, 0.0, A, B, p[4], n + cur[5]]
            pools.pop()
        pools.append(cur)
    return pools


def outputs(pools, m, T):
    c, s = [0.0] * T, [0.0] * T
    for i, (v, u, _, _, t0, l) in enumerate(pools):
        for k in range(l):
            c[t0 + k] = m.calc(v, u, k)
        if i >= 1:
            last, sec = m.tail(pools[i - 1])
            s[t0] = (c[t0] - m.g1 * last) - m.g2 * sec
    return c, s


def _rows(x, R):
    return np.broadcast_to(np.asarray(x, np.float64), (R,))


def deconvolve(y, d, r, lam=0.0, smin=0.0, base=None):
    """(R, T) float32 / float64 -> calcium float64 (R, T), spikes float64 (R, T), pools int32[R]."""
    y = np.asarray(y)
    R, T = y.shape
    lam, smin, base = _rows(lam, R), _rows(smin, R), _rows(0.0 if base is None else base, R)
    m = Model(d, r, T)
    c, s, n = np.empty((R, T)), np.empty((R, T)), np.empty(R, np.int32)
    for i in range(R):
        pools = forward(y[i], m, float(lam[i]), float(smin[i]), float(base[i]))
        c[i], s[i] = outputs(pools, m, T)
        n[i] = len(pools)
    return c, s, n


def rss(y, m, which, p, other):
    """RSS(p) of one trace: y as Python floats (a float32 input widened exactly)."""
    lam, smin = (p, other) if which == sr.LAM else (other, p)
    c, _ = outputs(forward(y, m, lam, smin), m, len(y))
    terms = []
    for a, b in zip(y, c):
        e = a - b
        terms.append(e * e)
    return sr.fold(terms)


def search(y, m, which, sigma, other=0.0, rounds=24):
    """_deconv_search_ref.search round for round, on this residual -> dict(param, rss, status, target)."""
    y = [float(v) for v in y]
    sigma, other = float(sigma), float(other)
    target = (sigma * sigma) * float(len(y))
    r0 = rss(y, m, which, 0.0, other)
    if not r0 < target:
        return dict(param=0.0, rss=r0, status=1, target=target)
    lo, rss_lo, hi, expanding = 0.0, r0, sigma, True
    for _ in range(rounds):
        p = hi if expanding else 0.5 * (lo + hi)
        q = rss(y, m, which, p, other)
        if q <= target:
            lo, rss_lo = p, q
            if expanding:
                hi = hi + hi
        else:
            hi, expanding = p, False
    return dict(param=lo, rss=rss_lo, status=2 if expanding else 0, target=target)


def constrained(y, d, r, which, sigma, other=0.0, rounds=24):
    """-> dict like _deconv_search_ref.deconvolve."""
    y = np.asarray(y)
    R, T = y.shape
    sigma, other = _rows(sigma, R), _rows(other, R)
    m = Model(d, r, T)
    out = dict(param=np.empty(R), rss=np.empty(R), target=np.empty(R), status=np.empty(R, np.int32), calcium=np.empty((R, T)),
               spikes=np.empty((R, T)), pools=np.empty(R, np.int32))
    for i in range(R):
        row = [float(v) for v in y[i]]
        s = search(row, m, which, float(sigma[i]), float(other[i]), rounds)
        lam, smin = (s['param'], float(other[i])) if which == sr.LAM else (float(other[i]), s['param'])
        pools = forward(row, m, lam, smin)
        out['calcium'][i], out['spikes'][i] = outputs(pools, m, T)
        out['pools'][i] = len(pools)
        for k in ('param', 'rss', 'target', 'status'):
            out[k][i] = s[k]
    return out


# ---- exact rationals -------------------------------------------------------------------------------------------------------------
def table_exact(d, r, T):
    g1, g2 = Fraction(d) + Fraction(r), -(Fraction(d) * Fraction(r))
    h = [Fraction(1), g1]
    for k in range(2, T + 1):
        h.append(g1 * h[k - 1] + g2 * h[k - 2])
    return g1, g2, h[:T + 1]


def forward_exact(y, d, r, lam=0, smin=0):
    """The same forward pass in Fractions: no rounding anywhere.  -> pools [v, u, A, B, t0, l], with v not clamped."""
    T = len(y)
    g1, g2, h = table_exact(d, r, T)
    H = lambda k: h[k] if k >= 0 else Fraction(0)                      # noqa: E731
    HH = lambda l: sum(h[k] * h[k] for k in range(l))                  # noqa: E731
    HP = lambda l: sum(h[k] * h[k - 1] for k in range(1, l))           # noqa: E731

    def calc(p, k):
        b = max(p[0], Fraction(0))
        return b if k == 0 else h[k] * b + g2 * h[k - 1] * p[1]

    pools = []
    for t in range(T):
        mu = lam * (1 - g1 - g2) if t < T - 2 else (lam * (1 - g1) if t == T - 2 else lam)
        cur = [None, None, Fraction(y[t]) - mu, Fraction(0), t, 1]
        while True:
            if not pools:
                cur[1] = Fraction(0)
                cur[0] = cur[2] / HH(cur[5])
                break
            p = pools[-1]
            last = calc(p, p[5] - 1)
            sec = calc(p, p[5] - 2) if p[5] >= 2 else p[1]
            cur[1] = last
            cur[0] = (cur[2] - g2 * last * HP(cur[5])) / HH(cur[5])
            if not cur[0] < g1 * last + g2 * sec + smin:
                break
            n = p[5]
            cur = [None, None, p[2] + h[n] * cur[2] + g2 * h[n - 1] * cur[3], p[3] + h[n - 1] * cur[2] + g2 * H(n - 2) * cur[3], p[4], n + cur[5]]
            pools.pop()
        pools.append(cur)
    return pools


# ---- the reach table ---------------------------------------------------------------------------------------------------------------
REACH_ROOTS = ROOTS[1]


def reach_trace(seed, sigma, T=1024):
    """_deconv_ref.reach_trace's events (the same random stream), convolved with the AR(2) kernel of REACH_ROOTS scaled to peak 1."""
    rs = np.random.RandomState(seed)
    sp = (rs.poisson(0.03, T) > 0)
    d, r = REACH_ROOTS
    k = np.arange(T)
    kernel = (d ** (k + 1) - r ** (k + 1)) / (d - r)                   # h in closed form
    c0 = np.convolve(sp, kernel / kernel.max())[:T]
    y = np.float32(c0 + sigma * rs.standard_normal(T))
    return sp, y


# ---- the library's host entry points ---------------------------------------------------------------------------------------------
def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _padded(y, pad):
    y = np.asarray(y)
    R, T = y.shape
    buf = np.full((R, T + pad), np.nan, y.dtype)
    buf[:, :T] = y
    return buf, R, T


def host_entry(L, y, d, r, lam=0.0, smin=0.0, base=None, pad=0):
    """dc_trace_deconv_ar2_host on the rows of y, stored with stride T + pad (the padding holds NaN), the table with rows of stride
    T + 1 + pad, outputs pre-filled with NaN.  -> calcium, spikes, pools."""
    from deep_calcium_amd.deconv import ar2_table
    buf, R, T = _padded(y, pad)
    H, _, _ = _padded(ar2_table(d, r, T), pad)
    g1, g2 = coefficients(float(d), float(r))
    lam, smin = _rows(lam, R).copy(), _rows(smin, R).copy()
    base = None if base is None else _rows(base, R).copy()
    c, s, n = np.full((R, T), np.nan), np.full((R, T), np.nan), np.full(R, -1, np.int32)
    L.dc_trace_deconv_ar2_host(_ptr(buf), int(buf.dtype == np.float64), T + pad, R, T, g1, g2, _ptr(H), T + 1 + pad, _ptr(lam), _ptr(smin),
                               _ptr(base), _ptr(c), _ptr(s), _ptr(n))
    return c, s, n


def host_constrained(L, y, d, r, which, sigma, other=0.0, rounds=24, pad=0):
    """dc_trace_deconv_ar2_constrained_host likewise -> dict like constrained() (without target)."""
    from deep_calcium_amd.deconv import ar2_table
    buf, R, T = _padded(y, pad)
    H, _, _ = _padded(ar2_table(d, r, T), pad)
    g1, g2 = coefficients(float(d), float(r))
    sigma, other = _rows(sigma, R).copy(), _rows(other, R).copy()
    out = dict(param=np.full(R, np.nan), rss=np.full(R, np.nan), status=np.full(R, -1, np.int32), calcium=np.full((R, T), np.nan),
               spikes=np.full((R, T), np.nan), pools=np.full(R, -1, np.int32))
    L.dc_trace_deconv_ar2_constrained_host(_ptr(buf), int(buf.dtype == np.float64), T + pad, R, T, g1, g2, _ptr(H), T + 1 + pad, which, _ptr(sigma),
                                           _ptr(other), rounds, _ptr(out['calcium']), _ptr(out['spikes']), _ptr(out['pools']), _ptr(out['param']),
                                           _ptr(out['rss']), _ptr(out['status']))
    return out


def same(got, want, what, names=sr.NAMES):
    for name in names:
        a, b = got[name], want[name]
        assert ref.same_bits(a, b), (name, what, np.argwhere(a != b)[:5].tolist())
