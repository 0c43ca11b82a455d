"""The oracle of the baseline in the AR(1) deconvolution (include/dcunet.h, "A baseline in the deconvolution") in plain Python
floats -- IEEE doubles, one rounding per operation, in the order the header writes them: the forward pass with a baseline, the
three folds RSS, S and A, the clamped Newton step, the fit at fixed parameters and the joint noise-constrained search round by
round.  Built on _deconv_ref (forward, outputs) and _deconv_search_ref (fold).  Also the dF/F generator of the reach table, built
on _deconv_ref.reach_trace and _dff_ref.baseline, and the ctypes calls of the library's host entry points that the CPU and the GPU
tests share."""
import ctypes

import numpy as np

import _deconv_ref as ref
import _deconv_search_ref as sr
import _dff_ref

SMIN, LAM = sr.SMIN, sr.LAM
FIT, PASS_A, PASS_B, PASS_LAST = 0, 1, 2, 3       # DC_TRACE_DECONV_BASE_*


def forward(y, G, lam, smin, b):
    """-> the final stack of pools of one trace; y as Python floats.  The pushed value is (y[t] - b) - mu."""
    T = len(y)
    g = G[1]
    pools = []
    for t in range(T):
        mu = lam * (1.0 - g) if t < T - 1 else lam
        pools.append([(y[t] - b) - mu, 1.0, t, 1])
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


def sums(y, G, pools, b):
    """-> (RSS, S, A) of a stack at the baseline b."""
    T = len(y)
    g = G[1]
    c, _ = ref.outputs(pools, G, T)
    a = [0.0] * T
    for v, _, t0, l in pools:
        if v > 0.0:
            u = (1.0 - G[l]) / (1.0 - g)
            q = (1.0 - G[l] * G[l]) / (1.0 - g * g)
            a[t0] = (u * u) / q
    d = [(y[t] - b) - c[t] for t in range(T)]
    return sr.fold([x * x for x in d]), sr.fold(d), sr.fold(a)


def step(b, S, A, T):
    den = 1.0 - A / float(T)
    if not den > 0.25:
        den = 0.25
    return b + (S / float(T)) / den


def fit(y, G, lam, smin, b0, rounds):
    """-> b_N, the trail [(b, S, A)] of the rounds."""
    b, trail = float(b0), []
    for _ in range(rounds):
        _, S, A = sums(y, G, forward(y, G, lam, smin, b), b)
        trail.append((b, S, A))
        b = step(b, S, A, len(y))
    return b, trail


def search(y, G, which, sigma, other=0.0, b0=0.0, rounds=24):
    """-> dict(param, base, rss, status, target, hi, trail): trail[i] = (p, b', r, lo, hi) after round i."""
    y = [float(v) for v in y]
    sigma, other, b = float(sigma), float(other), float(b0)
    T = len(y)
    target = (sigma * sigma) * float(T)

    def at(p, bb):
        lam, smin = (p, other) if which == LAM else (other, p)
        return sums(y, G, forward(y, G, lam, smin, bb), bb)
    r0 = at(0.0, b)[0]
    if not r0 < target:
        return dict(param=0.0, base=b, rss=r0, status=1, target=target, hi=None, trail=[(0.0, b, r0, 0.0, sigma)])
    lo, b_lo, rss_lo, hi, expanding = 0.0, b, r0, sigma, True
    trail = [(0.0, b, r0, lo, hi)]
    for _ in range(rounds):
        p = hi if expanding else 0.5 * (lo + hi)
        _, S, A = at(p, b)
        b = step(b, S, A, T)
        r = at(p, b)[0]
        if r <= target:
            lo, b_lo, rss_lo = p, b, r
            if expanding:
                hi = hi + hi
        else:
            hi, expanding = p, False
        trail.append((p, b, r, lo, hi))
    return dict(param=lo, base=b_lo, rss=rss_lo, status=2 if expanding else 0, target=target, hi=hi, trail=trail)


def _tables(gs, T):
    tables = {}
    for g in gs:
        if float(g) not in tables:
            tables[float(g)] = ref.table(float(g), T)
    return tables


def deconvolve(y, g, lam=0.0, smin=0.0, base=0.0, rounds=0):
    """The fit (rounds = 0: the given baseline).  (R, T) -> dict of calcium, spikes (R, T), pools int32[R], baseline float64[R].
    g: a scalar or one decay per row."""
    y = np.asarray(y)
    R, T = y.shape
    lam, smin, base, gs = (np.broadcast_to(np.asarray(x, np.float64), (R,)) for x in (lam, smin, base, g))
    tables = _tables(gs, T)
    out = dict(calcium=np.empty((R, T)), spikes=np.empty((R, T)), pools=np.empty(R, np.int32), baseline=np.empty(R))
    for r in range(R):
        G = tables[float(gs[r])]
        row = [float(v) for v in y[r]]
        b, _ = fit(row, G, float(lam[r]), float(smin[r]), float(base[r]), rounds)
        pools = forward(row, G, float(lam[r]), float(smin[r]), b)
        out['calcium'][r], out['spikes'][r] = ref.outputs(pools, G, T)
        out['pools'][r], out['baseline'][r] = len(pools), b
    return out


def deconvolve_search(y, g, which, sigma, other=0.0, base=0.0, rounds=24):
    """The joint search.  -> dict of param, baseline, rss, target float64[R], status int32[R], calcium, spikes, pools."""
    y = np.asarray(y)
    R, T = y.shape
    sigma, other, base, gs = (np.broadcast_to(np.asarray(x, np.float64), (R,)) for x in (sigma, other, base, g))
    tables = _tables(gs, T)
    out = dict(param=np.empty(R), baseline=np.empty(R), rss=np.empty(R), target=np.empty(R), status=np.empty(R, np.int32),
               calcium=np.empty((R, T)), spikes=np.empty((R, T)), pools=np.empty(R, np.int32))
    for r in range(R):
        G = tables[float(gs[r])]
        row = [float(v) for v in y[r]]
        s = search(row, G, which, float(sigma[r]), float(other[r]), float(base[r]), rounds)
        lam, smin = (s['param'], float(other[r])) if which == LAM else (float(other[r]), s['param'])
        pools = forward(row, G, lam, smin, s['base'])
        out['calcium'][r], out['spikes'][r] = ref.outputs(pools, G, T)
        out['pools'][r], out['baseline'][r] = len(pools), s['base']
        for k in ('param', 'rss', 'target', 'status'):
            out[k][r] = s[k]
    return out


FIT_NAMES = ('calcium', 'spikes', 'pools', 'baseline')
SEARCH_NAMES = ('calcium', 'spikes', 'pools', 'param', 'baseline', 'rss', 'status')


# ---- the dF/F of the reach table ---------------------------------------------------------------------------------------------------
def reach_dff(seed, sigma, T=1024, window=901, q=8):
    """The reach generator's trace as the dF/F the chain produces: F = round(1000 (1 + y)), F0 = the running q-th percentile by the
    integer rank rule over `window` frames, dF/F = (F - F0) / F0 in float32.  -> (spikes bool[T], dff float32[T], the true calcium
    float64[T])."""
    sp, y = ref.reach_trace(seed, sigma, T)
    calcium = np.convolve(sp, np.exp(-np.arange(T) / 8.0))[:T]
    F = np.rint(1000.0 * (1.0 + y.astype(np.float64))).astype(np.int64)[None]
    F0 = _dff_ref.baseline(F, window // 2, q)
    return sp, _dff_ref.dff(F, F0)[0], calcium


# ---- the library's host entry points -----------------------------------------------------------------------------------------------
def _host_tables(g, R, T, pad):
    """-> (G, ldG): one table (ldG = 0), or one row per trace of stride T + 1 + pad, the padding NaN."""
    from deep_calcium_amd.deconv import ar1_table
    if np.ndim(g) == 0:
        return ar1_table(float(g), T), 0
    G = np.full((R, T + 1 + pad), np.nan)
    for r in range(R):
        G[r, :T + 1] = ar1_table(float(g[r]), T)
    return G, T + 1 + pad


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def host_fit(L, y, g, lam=0.0, smin=0.0, base=0.0, rounds=0, pad=0):
    """dc_trace_deconv_ar1_fit_base_host on the rows of y, stored with stride T + pad (the padding holds NaN), outputs pre-filled
    with NaN / -1.  -> dict like deconvolve()."""
    y = np.asarray(y)
    R, T = y.shape
    buf = np.full((R, T + pad), np.nan, y.dtype)
    buf[:, :T] = y
    G, ldG = _host_tables(g, R, T, pad)
    lam, smin, b = (np.broadcast_to(np.asarray(x, np.float64), (R,)).copy() for x in (lam, smin, base))
    out = dict(calcium=np.full((R, T), np.nan), spikes=np.full((R, T), np.nan), pools=np.full(R, -1, np.int32), baseline=b)
    L.dc_trace_deconv_ar1_fit_base_host(_ptr(buf), int(y.dtype == np.float64), T + pad, R, T, _ptr(G), ldG, _ptr(lam), _ptr(smin), rounds,
                                        _ptr(out['calcium']), _ptr(out['spikes']), _ptr(out['pools']), _ptr(b))
    return out


def host_search(L, y, g, which, sigma, other=0.0, base=0.0, rounds=24, pad=0):
    """dc_trace_deconv_ar1_constrained_base_host likewise.  -> dict like deconvolve_search() (without target)."""
    y = np.asarray(y)
    R, T = y.shape
    buf = np.full((R, T + pad), np.nan, y.dtype)
    buf[:, :T] = y
    G, ldG = _host_tables(g, R, T, pad)
    sigma, other, b = (np.broadcast_to(np.asarray(x, np.float64), (R,)).copy() for x in (sigma, other, base))
    out = dict(param=np.full(R, np.nan), baseline=b, rss=np.full(R, np.nan), status=np.full(R, -1, np.int32), calcium=np.full((R, T), np.nan),
               spikes=np.full((R, T), np.nan), pools=np.full(R, -1, np.int32))
    L.dc_trace_deconv_ar1_constrained_base_host(_ptr(buf), int(y.dtype == np.float64), T + pad, R, T, _ptr(G), ldG, which, _ptr(sigma),
                                                _ptr(other), rounds, _ptr(out['calcium']), _ptr(out['spikes']), _ptr(out['pools']),
                                                _ptr(out['param']), _ptr(b), _ptr(out['rss']), _ptr(out['status']))
    return out
