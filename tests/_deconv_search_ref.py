"""The oracle of the noise-constrained search (include/dcunet.h, "Spikes by deconvolution", dc_trace_deconv_ar1_constrained) in
plain Python floats -- IEEE doubles, one rounding per operation, in the order the header writes them: the fixed-order fold, the
residual RSS(p), and the search round by round with its (lo, hi) trail.  Built on _deconv_ref.forward and _deconv_ref.outputs.
Also the reach generator's totals for a searched threshold and the ctypes call of the library's host entry point that the CPU
and the GPU tests share."""
import ctypes

import numpy as np

import _deconv_ref as ref

SMIN, LAM = 0, 1                      # DC_TRACE_DECONV_SEARCH_SMIN, DC_TRACE_DECONV_SEARCH_LAM
WHICH = {'s_min': SMIN, 'lam': LAM}
LANES = 256


def fold(terms):
    """fold(f, n) of the header: 256 lane sums over t = j, j + 256, ... from +0.0, then the tree h = 128 .. 1."""
    P = [0.0] * LANES
    for j in range(min(LANES, len(terms))):
        s = 0.0
        for x in terms[j::LANES]:
            s = s + x
        P[j] = s
    h = LANES // 2
    while h >= 1:
        for j in range(h):
            P[j] = P[j] + P[j + h]
        h //= 2
    return P[0]


def rss(y, G, which, p, other):
    """RSS(p) of one trace: y as Python floats (a float32 input widened exactly)."""
    lam, smin = (p, other) if which == LAM else (other, p)
    c, _ = ref.outputs(ref.forward(y, G, lam, smin), G, len(y))
    terms = []
    for a, b in zip(y, c):
        d = a - b
        terms.append(d * d)
    return fold(terms)


def search(y, G, which, sigma, other=0.0, rounds=24):
    """-> dict(param, rss, status, target, trail): trail[i] = (p, r, lo, hi) after round i, i = 0 .. rounds."""
    y = [float(v) for v in y]
    sigma, other = float(sigma), float(other)
    T = len(y)
    target = (sigma * sigma) * float(T)
    r0 = rss(y, G, which, 0.0, other)
    if not r0 < target:
        return dict(param=0.0, rss=r0, status=1, target=target, trail=[(0.0, r0, 0.0, sigma)], hi=None)
    lo, rss_lo, hi, expanding = 0.0, r0, sigma, True
    trail = [(0.0, r0, lo, hi)]
    for _ in range(rounds):
        p = hi if expanding else 0.5 * (lo + hi)
        r = rss(y, G, which, p, other)
        if r <= target:
            lo, rss_lo = p, r
            if expanding:
                hi = hi + hi
        else:
            hi, expanding = p, False
        trail.append((p, r, lo, hi))
    return dict(param=lo, rss=rss_lo, status=2 if expanding else 0, target=target, trail=trail, hi=hi)


def deconvolve(y, g, which, sigma, other=0.0, rounds=24):
    """(R, T) float32 / float64 -> dict of param, rss, target float64[R], status int32[R], calcium, spikes float64 (R, T), pools
    int32[R].  g: a scalar, or one decay per row (each row then has its own table)."""
    y = np.asarray(y)
    R, T = y.shape
    sigma = np.broadcast_to(np.asarray(sigma, np.float64), (R,))
    other = np.broadcast_to(np.asarray(other, np.float64), (R,))
    gs = np.broadcast_to(np.asarray(g, np.float64), (R,))
    out = dict(param=np.empty(R), rss=np.empty(R), target=np.empty(R), status=np.empty(R, np.int32), calcium=np.empty((R, T)),
               spikes=np.empty((R, T)), pools=np.empty(R, np.int32))
    tables = {}
    for r in range(R):
        gr = float(gs[r])
        if gr not in tables:
            tables[gr] = ref.table(gr, T)
        G = tables[gr]
        row = [float(v) for v in y[r]]
        s = search(row, G, which, float(sigma[r]), float(other[r]), rounds)
        lam, smin = (s['param'], float(other[r])) if which == LAM else (float(other[r]), s['param'])
        pools = ref.forward(row, G, lam, smin)
        out['calcium'][r], out['spikes'][r] = ref.outputs(pools, G, T)
        out['pools'][r] = len(pools)
        for k in ('param', 'rss', 'target', 'status'):
            out[k][r] = s[k]
    return out


NAMES = ('param', 'rss', 'status', 'calcium', 'spikes', 'pools')


# ---- the library's host entry point ----------------------------------------------------------------------------------------------
def host_entry(L, y, g, which, sigma, other=0.0, rounds=24, pad=0):
    """dc_trace_deconv_ar1_constrained_host on the rows of y, stored with stride T + pad (the padding holds NaN: it must not be read
    into a result), outputs pre-filled with NaN / -1.  -> dict like deconvolve() (without target)."""
    from deep_calcium_amd.deconv import ar1_table
    y = np.asarray(y)
    R, T = y.shape
    buf = np.full((R, T + pad), np.nan, y.dtype)
    buf[:, :T] = y
    G = ar1_table(g, T)
    sigma = np.broadcast_to(np.asarray(sigma, np.float64), (R,)).copy()
    other = np.broadcast_to(np.asarray(other, np.float64), (R,)).copy()
    out = dict(param=np.full(R, np.nan), rss=np.full(R, np.nan), status=np.full(R, -1, np.int32), calcium=np.full((R, T), np.nan),
               spikes=np.full((R, T), np.nan), pools=np.full(R, -1, np.int32))
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                  # noqa: E731
    L.dc_trace_deconv_ar1_constrained_host(ptr(buf), int(y.dtype == np.float64), T + pad, R, T, ptr(G), which, ptr(sigma), ptr(other), rounds,
                                           ptr(out['calcium']), ptr(out['spikes']), ptr(out['pools']), ptr(out['param']), ptr(out['rss']),
                                           ptr(out['status']))
    return out
