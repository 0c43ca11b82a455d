"""The oracle of the AR(2) coefficients (include/dcunet.h, "Trace dynamics: AR(2) coefficients"): the solve in plain Python floats --
IEEE doubles, one rounding per operation, evaluated in the order the header writes them -- on top of _dyn_ref's fold and
autocovariance; the roots and pick_roots restated independently of deep_calcium_amd.dynamics, trace by trace; and the ctypes call
of the library's host entry point that the CPU and the GPU tests share."""
import ctypes
import math

import numpy as np

import _dyn_ref as ref


def solve(xc, lags, sn, T):
    """xc: lags + 1 Python floats -> (g1_raw, g2_raw)."""
    c0 = xc[0] - sn * sn
    Saa = Sab = Sbb = Say = Sby = 0.0
    for i in range(lags):
        a = c0 if i == 0 else xc[i]
        b = xc[1] if i == 0 else (c0 if i == 1 else xc[i - 1])
        y = xc[i + 1]
        Saa = Saa + a * a
        Sab = Sab + a * b
        Sbb = Sbb + b * b
        Say = Say + a * y
        Sby = Sby + b * y
    det = Saa * Sbb - Sab * Sab
    if T < lags + 2 or not det > 0.0:
        return math.nan, math.nan
    g1 = (Say * Sbb - Sby * Sab) / det
    g2 = (Saa * Sby - Sab * Say) / det
    if not (math.isfinite(g1) and math.isfinite(g2)):
        return math.nan, math.nan
    return g1, g2


def solve_rows(xc, T, lags, sn):
    """xc float64 (R, lags + 1), sn float64[R] -> g12_raw float64 (R, 2)."""
    xc, sn = np.asarray(xc, np.float64), np.asarray(sn, np.float64)
    out = np.empty((xc.shape[0], 2))
    for r in range(xc.shape[0]):
        out[r] = solve([float(v) for v in xc[r]], lags, float(sn[r]), T)
    return out


def estimate(y, lags=10, sn=None):
    """(R, T) float32 / float64 -> sigma float64[R], xc float64 (R, lags + 1), g_raw float64[R], g12_raw float64 (R, 2)."""
    y = np.asarray(y)
    sigma, xc, g = ref.estimate(y, lags, sn=sn)
    noise = sigma if sn is None else np.broadcast_to(np.asarray(sn, np.float64), sigma.shape)
    return sigma, xc, g, solve_rows(xc, y.shape[1], lags, noise)


def roots(g1, g2):
    """-> (d, r), NaN where the discriminant is not positive."""
    disc = g1 * g1 + 4.0 * g2
    if not disc > 0.0:
        return math.nan, math.nan
    s = math.sqrt(disc)
    return (g1 + s) / 2.0, (g1 - s) / 2.0


def _median(v):
    v = sorted(v)
    n = len(v)
    return v[n // 2] if n & 1 else (v[n // 2 - 1] + v[n // 2]) / 2.0


def pick_roots(g12_raw, d_max=0.998, fallback=None):
    """The definition, one trace after the other: status 4 undefined; 1 disc <= 0 (or roots that round to one value); 3 d >= 1 or
    d > d_max; 2 r <= 0; 0 fine.  -> roots_each (R, 2), status int8[R], pooled (d, r)."""
    status, each = [], []
    for g1, g2 in np.asarray(g12_raw, np.float64).tolist():
        if not (math.isfinite(g1) and math.isfinite(g2)):
            status.append(4)
            each.append(None)
            continue
        d, r = roots(g1, g2)
        if not r < d:
            code = 1
        elif d >= 1.0 or d > d_max:
            code = 3
        elif r <= 0.0:
            code = 2
        else:
            code = 0
        status.append(code)
        each.append((d, r))
    fine = [e for e, s in zip(each, status) if s == 0]
    if fine:
        pooled = (_median([e[0] for e in fine]), _median([e[1] for e in fine]))
    elif fallback is not None:
        pooled = (float(fallback[0]), float(fallback[1]))
    else:
        raise ValueError('no trace of status 0 and no fallback')
    out = np.array([e if s == 0 else pooled for e, s in zip(each, status)], np.float64).reshape(-1, 2)
    return out, np.array(status, np.int8), pooled


# ---- a small recording of cells that have a rise time ----------------------------------------------------------------------------
def recording(seed, R=9, T=700, roots=(math.exp(-1.0 / 8), math.exp(-1.0 / 2)), amplitude=150.0, sigma=60.0):
    """(T, 5, 4 R + 1) int16, baseline 400: R cells of 3 x 3 pixels in a row, a blank column between them, each with its own Poisson
    events (rate 0.03 a frame) convolved with the AR(2) response of `roots` scaled to peak `amplitude`, on Gaussian pixel noise.
    -> frames, the ROIs as (9, 2) [y, x] arrays."""
    rs = np.random.RandomState(seed)
    d, r = roots
    k = np.arange(T)
    kernel = (d ** (k + 1) - r ** (k + 1)) / (d - r)
    kernel = kernel / kernel.max()
    f = 400.0 + sigma * rs.standard_normal((T, 5, 4 * R + 1))
    rois = []
    for i in range(R):
        trace = np.convolve(rs.poisson(0.03, T) > 0, kernel)[:T]
        x0 = 4 * i + 1
        f[:, 1:4, x0:x0 + 3] += amplitude * trace[:, None, None]
        rois.append(np.array([[y, x] for y in range(1, 4) for x in range(x0, x0 + 3)], np.int64))
    return np.rint(f).astype(np.int16), rois


# ---- the library's host entry point ----------------------------------------------------------------------------------------------
SENTINEL = -7.0                       # finite: NaN is a legal result


def host_entry(L, xc, T, lags, sn):
    """dc_trace_ar2_solve_host on xc (R, lags + 1) and sn [R]; the output pre-filled with a finite sentinel.  -> g12_raw (R, 2)."""
    xc = np.ascontiguousarray(xc, np.float64)
    R = xc.shape[0]
    assert xc.shape == (R, lags + 1)
    sn = np.ascontiguousarray(np.broadcast_to(np.asarray(sn, np.float64), (R,)))
    g12 = np.full((R, 2), SENTINEL)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                  # noqa: E731
    L.dc_trace_ar2_solve_host(ptr(xc), R, T, lags, ptr(sn), ptr(g12))
    return g12
