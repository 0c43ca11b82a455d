"""Trace dynamics on the device: the noise, the AR(1) decay and the AR(2) coefficients of every trace, estimated from the trace itself.

The deconvolution (deep_calcium_amd.deconv) needs the decay per frame g of the indicator, and a user rarely knows it to within a
factor of two: it depends on indicator, expression level, temperature and cell type.  This stage estimates it per trace from the
autocovariance (CaImAn's least squares for an AR(1) process, the noise removed at lag 0 only), together with the robust noise
sigma_hat that sets s_min -- trace_noise, computed where the dF/F lies.  The reference has no counterpart; the definitions in
include/dcunet.h ("Trace dynamics: noise and AR(1) decay") are the specification and csrc/trace_dyn_math.h is their one
implementation, so the results are defined bit for bit.

    kind      dtype     what
    noise     float64   sigma[R]: (1.4826 * med|d - med d|) / sqrt(2) of the first difference d; bit-equal to trace_noise
    autocov   float64   xc (R, lags + 1): xc_l = fold((y[t] - mean) (y[t+l] - mean), T - l) / T, the fold in a fixed order
    g_raw     float64   g_raw[R]: sum A_i xc_(i+1) / sum A_i A_i, A_0 = xc_0 - sn^2, A_i = xc_i; NaN where undefined

    dyn = TraceDynamics(tb.result_device('dff'), lags=5)
    sigma, g_raw = dyn.result('noise'), dyn.result('g_raw')
    g_each, status, g_pool = pick_gamma(g_raw)                       # host: clamp, replace the undefined, pool by the median
    dec = TraceDeconvolver(tb.result_device('dff'), g_pool, s_min=3.0 * sigma)       # or g_each: one decay per trace
    tau = ar1_tau(g_pool, fps=30.0)                                  # what that is in seconds

The rise: an indicator with a rise time is AR(2), c[t] = g1 c[t-1] + g2 c[t-2] + s[t], and TraceDynamicsAR2 estimates (g1, g2) per
trace from the same autocovariance -- CaImAn's estimate_time_constant(p=2): a least squares in two unknowns, the noise removed on
the diagonal (the header's "Trace dynamics: AR(2) coefficients"; dc_trace_ar2_solve runs after dc_trace_ar1_estimate on the same
stream, nothing is read back in between).  A single trace's estimate is poor -- a quarter to a half of them give complex roots --,
so the product is the pair pooled over the traces, which is exactly what the AR(2) deconvolution takes:

    g12_raw   float64   (R, 2): (g1_raw, g2_raw), NaN where undefined; not clamped, no roots taken

    dyn = TraceDynamicsAR2(tb.result_device('dff'), lags=10)
    roots_each, status, (d, r) = pick_roots(dyn.result('g12_raw'))   # host: the roots, which traces have usable ones, the medians
    dec = TraceDeconvolver(dyn.traces_device, d, rise=r, constrain='s_min', sigma=dyn.result_device('noise'))

Scope: one estimate per trace from the whole trace, lags up to 16; for AR(2) pooled roots only and real roots only.  Not built:
roots per trace in the deconvolution, refining the estimates by the deconvolution residual, noise from the power spectrum,
per-segment estimates, weights on the lags.

Importing this module needs neither torch nor the GPU; constructing a TraceDynamics does (there is no CPU fallback).
"""
import numpy as np

from ._matrix import _MatrixStage
from .deconv import _check_gamma, _check_roots, _check_traces, _per_trace

KINDS = ('noise', 'autocov', 'g_raw')
AR2_KINDS = KINDS + ('g12_raw',)      # of a TraceDynamicsAR2
LANES = 256                           # DC_TRACE_DYN_LANES: the width of the fold
MAX_LAGS = 16                         # DC_TRACE_DYN_MAX_LAGS
MAX_GROUPS = 8192                     # DC_TRACE_DYN_MAX_GROUPS: beyond, a workgroup walks several traces
FINE, RAISED, LOWERED, REPLACED = 0, 1, 2, 3          # the status codes of pick_gamma
ROOTS_FINE, ROOTS_COMPLEX, ROOTS_NO_RISE, ROOTS_SLOW, ROOTS_UNDEFINED = 0, 1, 2, 3, 4      # the status codes of pick_roots


def _check_kind(kind, kinds=KINDS):
    if kind not in kinds:
        raise ValueError('dynamics kind %r is not one of %s' % (kind, ', '.join(kinds)))


def _check_lags(lags, least=1):
    if isinstance(lags, (bool, np.bool_)) or not isinstance(lags, (int, np.integer)) or not least <= lags <= MAX_LAGS:
        raise ValueError('lags must be an integer in [%d, %d], not %r' % (least, MAX_LAGS, lags))
    return int(lags)


# ---- the host helpers: definitions, float64 numpy -----------------------------------------------------------------------------------
def ar1_tau(g, fps):
    """tau = -1 / (fps * log(g)): the decay time in seconds of the decay per frame g at fps frames a second; the inverse of ar1_gamma."""
    g = _check_gamma(g)
    try:
        fps = float(fps)
    except (TypeError, ValueError):
        raise ValueError('fps must be a number, not %r' % (fps,))
    if not 0.0 < fps < np.inf:
        raise ValueError('fps must be positive and finite, not %r' % (fps,))
    return float(-1.0 / (fps * np.log(g)))


def pick_gamma(g_raw, g_min=0.05, g_max=0.998, fallback=None):
    """-> (g_each float64[R], status int8[R], g_pool float).  g_raw: the raw estimates of R traces, NaN (or any value that is not
    finite) where undefined.  g_pool is np.median of the defined ones, clamped to [g_min, g_max]; g_each is g_raw clamped, an
    undefined entry replaced by `fallback`, which defaults to g_pool.  status: 0 fine, 1 raised to g_min, 2 lowered to g_max,
    3 replaced.  With no defined trace g_pool is the fallback; without one either that is a ValueError."""
    try:
        raw = np.asarray(g_raw, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('g_raw must be numbers, not %r' % (g_raw,))
    if raw.ndim != 1 or raw.size < 1:
        raise ValueError('g_raw must hold one value per trace, not shape %r' % (raw.shape,))
    g_min, g_max = _check_gamma(g_min), _check_gamma(g_max)
    if g_min > g_max:
        raise ValueError('g_min = %r is above g_max = %r' % (g_min, g_max))
    if fallback is not None:
        fallback = _check_gamma(fallback)
    defined = np.isfinite(raw)
    if defined.any():
        g_pool = float(min(max(float(np.median(raw[defined])), g_min), g_max))
    elif fallback is not None:
        g_pool = fallback
    else:
        raise ValueError('no trace has a defined decay (trace 0: g_raw = %r) and there is no fallback' % (float(raw[0]),))
    status = np.zeros(raw.shape, np.int8)
    status[defined & (raw < g_min)] = RAISED
    status[defined & (raw > g_max)] = LOWERED
    status[~defined] = REPLACED
    g_each = np.where(defined, np.minimum(np.maximum(raw, g_min), g_max), g_pool if fallback is None else fallback)
    return np.ascontiguousarray(g_each, dtype=np.float64), status, g_pool


def ar2_roots(g1, g2):
    """-> (d, r), float64: the roots of x^2 = g1 x + g2, disc = g1 * g1 + 4 * g2, d = (g1 + sqrt(disc)) / 2 the decay and
    r = (g1 - sqrt(disc)) / 2 the rise; NaN where disc <= 0 (complex or equal roots) or an input is NaN.  The inverse of
    deep_calcium_amd.deconv.ar2_coefficients."""
    try:
        g1, g2 = np.asarray(g1, dtype=np.float64), np.asarray(g2, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('g1 and g2 must be numbers, not %r and %r' % (g1, g2))
    if g1.shape != g2.shape:
        raise ValueError('g1 and g2 must have one shape, not %r and %r' % (g1.shape, g2.shape))
    disc = g1 * g1 + 4.0 * g2
    real = disc > 0.0                                                # NaN fails the comparison
    root = np.sqrt(np.where(real, disc, 0.0))
    d = np.where(real, (g1 + root) / 2.0, np.nan)
    r = np.where(real, (g1 - root) / 2.0, np.nan)
    return d[()], r[()]


def _check_pick_roots(d_max, fallback):
    """The bound and the fallback of pick_roots -> (d_max, fallback as floats or None)."""
    d_max = _check_gamma(d_max)
    if fallback is not None:
        try:
            fd, fr = fallback
        except (TypeError, ValueError):
            raise ValueError('fallback must be a pair of roots (d, r), not %r' % (fallback,))
        fallback = _check_roots(fd, fr)
    return d_max, fallback


def pick_roots(g12_raw, d_max=0.998, fallback=None):
    """-> (roots_each float64 (R, 2), status int8[R], pooled (d, r) floats).  g12_raw: (R, 2), the raw coefficients (g1, g2) of R
    traces, NaN (or any value that is not finite) where undefined.  status, the first that applies: 4 undefined; 1 disc <= 0,
    complex or equal roots; 3 d >= 1 or d > d_max, no decay within the recording; 2 r <= 0, the trace is AR(1) by this estimate;
    0 fine, 0 < r < d <= d_max.  pooled: the median of d and the median of r over the traces of status 0 -- a single estimate is
    poor, the pooled pair is the product.  roots_each: a trace's own (d, r) where its status is 0, the pooled pair elsewhere.
    With no trace of status 0 pooled is `fallback` = (d, r); without one either that is a ValueError."""
    try:
        raw = np.asarray(g12_raw, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('g12_raw must be numbers, not %r' % (g12_raw,))
    if raw.ndim != 2 or raw.shape[0] < 1 or raw.shape[1] != 2:
        raise ValueError('g12_raw must hold (g1, g2) per trace, shape (R, 2), not %r' % (raw.shape,))
    d_max, fallback = _check_pick_roots(d_max, fallback)
    g1, g2 = raw[:, 0], raw[:, 1]
    defined = np.isfinite(g1) & np.isfinite(g2)
    with np.errstate(invalid='ignore', over='ignore'):
        d, r = ar2_roots(g1, g2)
        real = defined & (r < d)                                     # disc > 0, and roots that differ after rounding
        status = np.full(raw.shape[0], ROOTS_FINE, np.int8)
        status[real & (r <= 0.0)] = ROOTS_NO_RISE
        status[real & ((d >= 1.0) | (d > d_max))] = ROOTS_SLOW
    status[defined & ~real] = ROOTS_COMPLEX
    status[~defined] = ROOTS_UNDEFINED
    fine = status == ROOTS_FINE
    if fine.any():
        pooled = (float(np.median(d[fine])), float(np.median(r[fine])))
        assert 0.0 < pooled[1] < pooled[0] <= d_max, pooled          # r_i < d_i for every one of them, so for the medians
    elif fallback is not None:
        pooled = fallback
    else:
        raise ValueError('no trace gives two real roots in (0, 1) (trace 0: g1_raw = %r, g2_raw = %r) and there is no fallback: '
                         'give tau and tau_rise' % (float(g1[0]), float(g2[0])))
    roots_each = np.where(fine[:, None], np.stack([d, r], axis=1), np.array(pooled)[None])
    return np.ascontiguousarray(roots_each, dtype=np.float64), status, pooled


class TraceDynamics(_MatrixStage):
    """Owns the device state of one estimate: the traces and the three results -- four with order=2, which adds the AR(2)
    coefficients.  The kernels run at most once; result() only copies."""
    _noun = 'estimate'

    def __init__(self, traces, lags=5, sn=None, device=None, order=1):
        """traces: (R, T) float32 or float64, numpy (checked for non-finite values) or a tensor already on the device (read in
        place, never written; THE CALLER PROMISES FINITE VALUES).  lags in [1, 16].  sn: None -- the noise that is removed at lag 0
        is the trace's own sigma_hat -- or a scalar or one value per trace, >= 0.  order: 1, or 2 -- what TraceDynamicsAR2 makes:
        dc_trace_ar2_solve then runs behind the estimate on the same stream, on the xc and the noise it wrote (or on sn), the
        kinds are AR2_KINDS and lags is in [2, 16]."""
        # ---- everything that can be wrong with the arguments is a ValueError before the library or the GPU is touched ----
        R, T, f64 = _check_traces(traces)
        if isinstance(order, (bool, np.bool_)) or order not in (1, 2):
            raise ValueError('order must be 1 or 2, not %r' % (order,))
        self.order = int(order)
        self.kinds = KINDS if self.order == 1 else AR2_KINDS
        self.lags = _check_lags(lags, self.order)
        sn = None if sn is None else _per_trace(sn, 'sn', R)
        self.n_traces, self.n_frames = R, T

        self._open(device, like=traces)
        self.traces_device = self._resident(traces, 'traces')      # what a TraceDeconvolver can be given next: no second upload
        self._f64 = f64
        self._ld = self._row_stride(self.traces_device, T)
        self._sn = None if sn is None else self._resident(sn, 'sn')
        self._out = None

    def _run(self):
        """Everything is enqueued by one call: nothing is read back between the estimate and the solve."""
        if self._out is None:
            R, T = self.n_traces, self.n_frames
            sigma, xc, g_raw = self._empty(R, 'float64'), self._empty((R, self.lags + 1), 'float64'), self._empty(R, 'float64')
            out = dict(noise=sigma, autocov=xc, g_raw=g_raw)
            if self.order == 2:
                out['g12_raw'] = self._empty((R, 2), 'float64')
            with self._torch.cuda.device(self.device):
                stream = self._stream()
                self.L.dc_trace_ar1_estimate(self.traces_device.data_ptr(), int(self._f64), self._ld, R, T, self.lags,
                                             None if self._sn is None else self._sn.data_ptr(), sigma.data_ptr(), xc.data_ptr(),
                                             g_raw.data_ptr(), stream)
                if self.order == 2:
                    noise = sigma if self._sn is None else self._sn
                    self.L.dc_trace_ar2_solve(xc.data_ptr(), R, T, self.lags, noise.data_ptr(), out['g12_raw'].data_ptr(), stream)
            self._out = out
        return self._out

    def result_device(self, kind=None):
        """result(kind) as a tensor on the device (the object's own state: do not write to it): float64, [R] for 'noise' and
        'g_raw', (R, lags + 1) for 'autocov', and with order=2 (R, 2) for 'g12_raw'.  kind=None: 'g_raw', or 'g12_raw' with order=2."""
        if kind is None:
            kind = self.kinds[-1]
        _check_kind(kind, self.kinds)
        return self._run()[kind]


def TraceDynamicsAR2(traces, lags=10, sn=None, device=None):
    """-> a TraceDynamics of order 2: dc_trace_ar1_estimate, then dc_trace_ar2_solve on what it wrote, on the same stream; nothing
    is read back in between.  Its kinds are AR2_KINDS, result() gives 'g12_raw', float64 (R, 2): (g1_raw, g2_raw) per trace.  lags
    in [2, 16]; sn as for TraceDynamics: it is also the noise that leaves the diagonal of the AR(2) system.  (A function, not a
    class: the stage is TraceDynamics.)"""
    return TraceDynamics(traces, lags=lags, sn=sn, device=device, order=2)


def estimate_ar1_device(traces, lags=5, sn=None, g_min=0.05, g_max=0.998, fallback=None, device=None):
    """-> dict(g_each=, status=, g_pool=, g_raw=, sigma=, autocov=): TraceDynamics on the traces, then pick_gamma on its g_raw."""
    _check_traces(traces)
    _check_lags(lags)
    pick_gamma(np.array([0.5]), g_min, g_max, fallback)          # the bounds, before the GPU is touched
    dyn = TraceDynamics(traces, lags=lags, sn=sn, device=device)
    g_raw = dyn.result('g_raw')
    g_each, status, g_pool = pick_gamma(g_raw, g_min, g_max, fallback)
    return dict(g_each=g_each, status=status, g_pool=g_pool, g_raw=g_raw, sigma=dyn.result('noise'), autocov=dyn.result('autocov'))


def estimate_ar2_device(traces, lags=10, sn=None, d_max=0.998, fallback=None, device=None):
    """-> dict(roots_each=, status=, pooled=, g12_raw=, g_raw=, sigma=, autocov=): TraceDynamicsAR2 on the traces, then pick_roots
    on its g12_raw."""
    _check_traces(traces)
    _check_lags(lags, 2)
    _check_pick_roots(d_max, fallback)                             # the bound and the fallback, before the GPU is touched
    dyn = TraceDynamicsAR2(traces, lags=lags, sn=sn, device=device)
    g12_raw = dyn.result('g12_raw')
    roots_each, status, pooled = pick_roots(g12_raw, d_max, fallback)
    return dict(roots_each=roots_each, status=status, pooled=pooled, g12_raw=g12_raw, g_raw=dyn.result('g_raw'), sigma=dyn.result('noise'),
                autocov=dyn.result('autocov'))
