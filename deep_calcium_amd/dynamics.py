"""Trace dynamics on the device: the noise and the AR(1) decay of every trace, estimated from the trace itself.

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

Scope: AR(1), one estimate per trace from the whole trace, lags up to 16.  Not built: AR(2), refining g by the deconvolution
residual, noise from the power spectrum, per-segment estimates, weights on the lags.

Importing this module needs neither torch nor the GPU; constructing a TraceDynamics does (there is no CPU fallback).
"""
import numpy as np

from ._matrix import _MatrixStage
from .deconv import _check_gamma, _check_traces, _per_trace

KINDS = ('noise', 'autocov', 'g_raw')
LANES = 256                           # DC_TRACE_DYN_LANES: the width of the fold
MAX_LAGS = 16                         # DC_TRACE_DYN_MAX_LAGS
MAX_GROUPS = 8192                     # DC_TRACE_DYN_MAX_GROUPS: beyond, a workgroup walks several traces
FINE, RAISED, LOWERED, REPLACED = 0, 1, 2, 3          # the status codes of pick_gamma


def _check_kind(kind):
    if kind not in KINDS:
        raise ValueError('dynamics kind %r is not one of %s' % (kind, ', '.join(KINDS)))


def _check_lags(lags):
    if isinstance(lags, (bool, np.bool_)) or not isinstance(lags, (int, np.integer)) or not 1 <= lags <= MAX_LAGS:
        raise ValueError('lags must be an integer in [1, %d], not %r' % (MAX_LAGS, lags))
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


class TraceDynamics(_MatrixStage):
    """Owns the device state of one estimate: the traces and the three results.  The kernel runs at most once; result() only copies."""
    _noun = 'estimate'

    def __init__(self, traces, lags=5, sn=None, device=None):
        """traces: (R, T) float32 or float64, numpy (checked for non-finite values) or a tensor already on the device (read in
        place, never written; THE CALLER PROMISES FINITE VALUES).  lags in [1, 16].  sn: None -- the noise that is removed at lag 0
        is the trace's own sigma_hat -- or a scalar or one value per trace, >= 0."""
        # ---- everything that can be wrong with the arguments is a ValueError before the library or the GPU is touched ----
        R, T, f64 = _check_traces(traces)
        self.lags = _check_lags(lags)
        sn = None if sn is None else _per_trace(sn, 'sn', R)
        self.n_traces, self.n_frames = R, T

        self._open(device, like=traces)
        self.traces_device = self._resident(traces, 'traces')      # what a TraceDeconvolver can be given next: no second upload
        self._f64 = f64
        self._ld = self._row_stride(self.traces_device, T)
        self._sn = None if sn is None else self._resident(sn, 'sn')
        self._out = None

    def _run(self):
        if self._out is None:
            R, T = self.n_traces, self.n_frames
            sigma, xc, g_raw = self._empty(R, 'float64'), self._empty((R, self.lags + 1), 'float64'), self._empty(R, 'float64')
            with self._torch.cuda.device(self.device):
                self.L.dc_trace_ar1_estimate(self.traces_device.data_ptr(), int(self._f64), self._ld, R, T, self.lags,
                                             None if self._sn is None else self._sn.data_ptr(), sigma.data_ptr(), xc.data_ptr(),
                                             g_raw.data_ptr(), self._stream())
            self._out = dict(noise=sigma, autocov=xc, g_raw=g_raw)
        return self._out

    def result_device(self, kind='g_raw'):
        """result(kind) as a tensor on the device (the object's own state: do not write to it): float64, [R] for 'noise' and
        'g_raw', (R, lags + 1) for 'autocov'."""
        _check_kind(kind)
        return self._run()[kind]


def estimate_ar1_device(traces, lags=5, sn=None, g_min=0.05, g_max=0.998, fallback=None, device=None):
    """-> dict(g_each=, status=, g_pool=, g_raw=, sigma=, autocov=): TraceDynamics on the traces, then pick_gamma on its g_raw."""
    _check_traces(traces)
    _check_lags(lags)
    pick_gamma(np.array([0.5]), g_min, g_max, fallback)          # the bounds, before the GPU is touched
    dyn = TraceDynamics(traces, lags=lags, sn=sn, device=device)
    g_raw = dyn.result('g_raw')
    g_each, status, g_pool = pick_gamma(g_raw, g_min, g_max, fallback)
    return dict(g_each=g_each, status=status, g_pool=g_pool, g_raw=g_raw, sigma=dyn.result('noise'), autocov=dyn.result('autocov'))
