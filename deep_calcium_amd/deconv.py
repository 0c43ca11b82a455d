"""Spikes by deconvolution on the device: non-negative AR(1) deconvolution of dF/F traces, without a trained model.

The last stage of the chain for a user who has no UNet1D model file.  Calcium c[t] = g c[t-1] + s[t] with s >= 0 is fitted to every
trace by an OASIS-style pool-merging forward pass; the reference has no counterpart, the definitions in include/dcunet.h ("Spikes by
deconvolution") are the specification, and csrc/deconv_math.h is their one implementation: IEEE double operations in a fixed order,
so the results are defined bit for bit.

    kind      dtype     what
    calcium   float64   c: per pool, b G[k] with b = max(v, +0.0)
    spikes    float64   s = c[t] - g c[t-1] at the first frame of every pool but the first, +0.0 elsewhere; an event is s > 0
    pools     int32     the number of pools of each trace

    g = ar1_gamma(tau=1.0, fps=30.0)
    dec = TraceDeconvolver(tb.result_device('dff'), g, s_min=3.0 * trace_noise(tb.result('dff')), lam=0.0)
    c, s, n = dec.result('calcium'), dec.result('spikes'), dec.result('pools')

    c, s = deconvolve_traces_device('dataset.hdf5', rois, window=1801, tau=1.0, fps=30.0, k=3.0)    # dff_traces_device, then the above

    c, s, info = deconvolve_traces_device('dataset.hdf5', rois, window=1801, tau='auto', details=True)     # g estimated from the traces
    dec = TraceDeconvolver(dff_dev, g_each, s_min=3.0 * sigma)          # one decay per trace (deep_calcium_amd.dynamics.pick_gamma)

The threshold without a k: constrain='s_min' (or 'lam') searches that parameter per trace, on the device, for the largest value
tried whose residual stays within the noise, RSS(p) <= sigma^2 T (the header's "noise-constrained search"); the object then also
gives

    param     float64   p*, the value found
    rss       float64   RSS(p*)
    target    float64   (sigma * sigma) * T
    status    int32     0 bracketed, 1 p* = 0 (the residual reaches the noise unconstrained), 2 never bracketed (slack at p*)

    dec = TraceDeconvolver(dff_dev, g, constrain='s_min')               # sigma = the trace noise, computed on the device
    c, s, info = deconvolve_traces_device('dataset.hdf5', rois, window=1801, tau='auto', k='noise', details=True)

Search s_min for events (spikes > 0) and lam for a denoised calcium: the L1 solution's spikes > 0 is a poor event detector.

A baseline: dF/F over a low rolling percentile sits about one noise sigma above zero in its quiet stretches, and the non-negative
model pays for a constant with spurious spikes.  baseline= takes one constant per trace off the data inside the forward pass --
given, or with 'fit' estimated on the device (the header's "A baseline in the deconvolution": a clamped Newton step on the mean
residual, baseline_rounds of them at fixed parameters, or one a round inside the noise-constrained search).  calcium stays c,
without the baseline: the fitted trace is c + baseline.

    baseline  float64   b per trace: the values used (zeros without baseline=)

    dec = TraceDeconvolver(dff_dev, g, constrain='s_min', baseline='fit')        # threshold and baseline found together: recommended
    c, s, info = deconvolve_traces_device('dataset.hdf5', rois, window=1801, tau='auto', k='noise', baseline='fit', details=True)

With a fixed threshold the fit is only as good as the threshold: one that is too high misses events, whose fluorescence is then
absorbed into the baseline.

A rise time: rise=r makes the model AR(2), c[t] = g1 c[t-1] + g2 c[t-2] + s[t] with the roots g (the decay) and r (the rise) per
frame, g1 = g + r, g2 = -(g * r) (the header's "A rise time in the deconvolution"; csrc/deconv_ar2_math.h).  An indicator that
takes several frames to peak is otherwise explained as a run of spikes.  Everything above works as it does without it, except
baseline='fit' and a decay per trace; the greedy pass is feasible but, unlike AR(1), not promised to be optimal.

    dec = TraceDeconvolver(dff_dev, ar1_gamma(1.0, 30.0), rise=ar1_gamma(0.1, 30.0), constrain='s_min')
    c, s = deconvolve_traces_device('dataset.hdf5', rois, window=1801, tau=1.0, tau_rise=0.1, fps=30.0, k='noise')
    c, s = deconvolve_traces_device('dataset.hdf5', rois, window=1801, tau='auto', tau_rise='auto', k='noise')   # both roots estimated

(deep_calcium_amd.dynamics: TraceDynamicsAR2 and pick_roots estimate the pair of roots from the traces and pool it.)

Not built: fitting the baseline under AR(2), a pair of roots per trace, complex or equal roots, OASIS's
corrective passes; optimising g by the residual, a time-varying baseline; for the search: both parameters at once, a warm start,
the closed-form lam update of OASIS, a joint search over g.

Importing this module needs neither torch nor the GPU; constructing a TraceDeconvolver does (there is no CPU fallback).
"""
import numpy as np

from ._matrix import _MatrixStage, _check_matrix, _is_device_tensor

KINDS = ('calcium', 'spikes', 'pools')
SEARCH_KINDS = ('param', 'rss', 'target', 'status')       # of a constrained object only
CONSTRAIN = {'s_min': 0, 'lam': 1}    # DC_TRACE_DECONV_SEARCH_SMIN, DC_TRACE_DECONV_SEARCH_LAM
MAX_ROUNDS = 64                       # DC_TRACE_DECONV_SEARCH_MAX_ROUNDS
MAX_BASELINE_ROUNDS = 64              # DC_TRACE_DECONV_BASE_MAX_ROUNDS
MAX_SIGMA = 2.0 ** 500
MAX_FRAMES = 1 << 24                  # DC_TRACE_DECONV_MAX_FRAMES
MAX_SAMPLES = 1 << 31                 # DC_TRACE_DECONV_MAX_SAMPLES


def _check_kind(kind, constrained=False):
    if constrained and kind in SEARCH_KINDS:
        return
    if kind not in KINDS:
        raise ValueError('deconvolution kind %r is not one of %s' % (kind, ', '.join(KINDS)))


def _check_rounds(rounds, name, limit):
    if isinstance(rounds, (bool, np.bool_)) or not isinstance(rounds, (int, np.integer)) or not 1 <= rounds <= limit:
        raise ValueError('%s must be an integer in [1, %d], not %r' % (name, limit, rounds))
    return int(rounds)


def _check_device_vector(x, what, R):
    if not x.is_cuda or str(x.dtype) != 'torch.float64' or tuple(x.shape) != (R,) or not x.is_contiguous():
        raise ValueError('%s must be a contiguous float64 tensor of %d values on the device, not %s %r' % (what, R, x.dtype, tuple(x.shape)))


def _check_baseline(baseline, rounds, R, constrained):
    """baseline= of TraceDeconvolver -> None (the default: no baseline at all), 'fit', a float64[R] array or a device tensor."""
    if isinstance(baseline, str):
        if baseline != 'fit':
            raise ValueError("baseline must be a number, one value per trace or 'fit', not %r" % (baseline,))
        _check_rounds(rounds, 'baseline_rounds', MAX_BASELINE_ROUNDS)
        return 'fit'
    if _is_device_tensor(baseline):
        _check_device_vector(baseline, 'baseline', R)
    else:
        try:
            a = np.asarray(baseline, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("baseline must be a number, one value per trace or 'fit', not %r" % (baseline,))
        if a.ndim == 0:
            if float(a) == 0.0:
                return None
            a = np.full(R, float(a), np.float64)
        if a.shape != (R,):
            raise ValueError('baseline must be a scalar or one value per trace (%d), not shape %r' % (R, a.shape))
        bad = np.flatnonzero(~np.isfinite(a))
        if bad.size:
            raise ValueError('baseline must be finite: trace %d has %r' % (int(bad[0]), float(a[bad[0]])))
        baseline = np.ascontiguousarray(a)
    if constrained:
        raise ValueError("a given baseline cannot go with constrain=: the search fits it (baseline='fit') or has none")
    return baseline


def _check_sigma(sigma, R):
    """The noise the search is held to: a scalar or one value per trace, finite, >= 0 and below 2**500 -> float64[R]."""
    sigma = _per_trace(sigma, 'sigma', R)
    bad = np.flatnonzero(sigma >= MAX_SIGMA)
    if bad.size:
        raise ValueError('sigma must be below 2**500: trace %d has %r' % (int(bad[0]), float(sigma[bad[0]])))
    return sigma


# ---- the host helpers: definitions, float64 numpy -----------------------------------------------------------------------------------
def ar1_gamma(tau, fps):
    """g = exp(-1 / (tau * fps)): the decay per frame of an indicator whose decay time is tau seconds, recorded at fps frames a second."""
    try:
        tau, fps = float(tau), float(fps)
    except (TypeError, ValueError):
        raise ValueError('tau and fps must be numbers, not %r and %r' % (tau, fps))
    if not (0.0 < tau < np.inf and 0.0 < fps < np.inf):
        raise ValueError('tau and fps must be positive and finite, not %r and %r' % (tau, fps))
    return _check_gamma(float(np.exp(-1.0 / (tau * fps))))


def _check_gamma(g):
    try:
        g = float(g)
    except (TypeError, ValueError):
        raise ValueError('g must be a number in (0, 1), not %r' % (g,))
    if not 0.0 < g < 1.0:                      # NaN fails both comparisons
        raise ValueError('g must be inside (0, 1), not %r' % (g,))
    return g


def ar1_table(g, T):
    """G, float64[T + 1]: G[0] = 1, G[l] = G[l-1] * g by repeated multiplication (never pow: the table IS the definition)."""
    g = _check_gamma(g)
    if isinstance(T, (bool, np.bool_)) or not isinstance(T, (int, np.integer)) or T < 0:
        raise ValueError('T must be a non-negative integer, not %r' % (T,))
    G = np.empty(int(T) + 1, np.float64)
    G[0] = 1.0
    G[1:] = g
    return np.multiply.accumulate(G)           # a sequential left fold: G[l] = G[l-1] * g


def _check_roots(g, rise):
    """The roots of the AR(2) model, decay and rise per frame: scalars, 0 < rise < g < 1 -> (g, rise) as floats."""
    if np.ndim(g) != 0:
        raise ValueError('a decay per trace is not built for AR(2): with rise=, g must be a scalar')
    g = _check_gamma(g)
    try:
        if np.ndim(rise) != 0:
            raise TypeError
        rise = float(rise)
    except (TypeError, ValueError):
        raise ValueError('rise must be a number in (0, g), not %r' % (rise,))
    if not 0.0 < rise < g:                     # NaN fails both comparisons
        raise ValueError('rise must be inside (0, g = %r), not %r' % (g, rise))
    return g, rise


def ar2_coefficients(g, rise):
    """g1 = g + rise, g2 = -(g * rise): the coefficients of c[t] = g1 c[t-1] + g2 c[t-2] + s[t] whose roots are g and rise."""
    g, rise = _check_roots(g, rise)
    return g + rise, -(g * rise)


def ar2_table(g, rise, T):
    """float64 (3, T + 1), the rows h, HH and HP of the header: h[0] = 1, h[1] = g1, h[k] = g1 * h[k-1] + g2 * h[k-2]; HH[0] = HP[0] =
    0, HH[l+1] = HH[l] + h[l] * h[l], HP[l+1] = HP[l] + h[l] * h[l-1] (the term of l = 0 is +0.0).  The table IS the definition."""
    g1, g2 = ar2_coefficients(g, rise)
    if isinstance(T, (bool, np.bool_)) or not isinstance(T, (int, np.integer)) or T < 0:
        raise ValueError('T must be a non-negative integer, not %r' % (T,))
    T = int(T)
    h = [1.0, g1]
    for k in range(2, T + 1):                  # plain floats: one rounding per operation, in this order
        h.append(g1 * h[k - 1] + g2 * h[k - 2])
    H = np.zeros((3, T + 1), np.float64)
    H[0] = h[:T + 1]
    if T:
        prod = np.zeros(T, np.float64)
        H[1, 1:] = np.add.accumulate(H[0, :T] * H[0, :T])              # a sequential left fold, like ar1_table's
        prod[1:] = H[0, 1:T] * H[0, :T - 1]
        H[2, 1:] = np.add.accumulate(prod)
    return H


def ar2_peak(g, rise):
    """The frame at which the response h to one spike peaks: the first k with h[k+1] <= h[k]."""
    g1, g2 = ar2_coefficients(g, rise)
    a, b, k = 1.0, g1, 0
    while b > a:
        a, b, k = b, g1 * b + g2 * a, k + 1
    return k


def trace_noise(y):
    """Per row of an (R, T) matrix: d = diff(float64(y)), sigma = 1.4826 * median(|d - median(d)|) / sqrt(2), the robust noise of
    the trace from its first difference.  0.0 for T < 3.  float64[R]."""
    y = np.asarray(y)
    if y.ndim != 2 or y.dtype.kind not in 'fiu':
        raise ValueError('traces must be a numeric (R, T) matrix, not %s %r' % (y.dtype, y.shape))
    R, T = y.shape
    if T < 3:
        return np.zeros(R, np.float64)
    d = np.diff(y.astype(np.float64), axis=1)
    return 1.4826 * np.median(np.abs(d - np.median(d, axis=1, keepdims=True)), axis=1) / np.sqrt(2.0)


def _per_trace(x, what, R):
    """A scalar or a length-R array of finite doubles >= 0 -> float64[R]."""
    try:
        a = np.asarray(x, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('%s must be a number or %d numbers, not %r' % (what, R, x))
    if a.ndim == 0:
        a = np.full(R, float(a), np.float64)
    if a.shape != (R,):
        raise ValueError('%s must be a scalar or one value per trace (%d), not shape %r' % (what, R, a.shape))
    bad = np.flatnonzero(~(np.isfinite(a) & (a >= 0.0)))
    if bad.size:
        raise ValueError('%s must be finite and >= 0: trace %d has %r' % (what, int(bad[0]), float(a[bad[0]])))
    return np.ascontiguousarray(a)


def _per_trace_gamma(g, R):
    """One decay per trace, each inside (0, 1) -> float64[R]."""
    try:
        a = np.asarray(g, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('g must be a number or %d numbers in (0, 1), not %r' % (R, g))
    if a.shape != (R,):
        raise ValueError('g must be a scalar or one value per trace (%d), not shape %r' % (R, a.shape))
    bad = np.flatnonzero(~((a > 0.0) & (a < 1.0)))                 # NaN fails both comparisons
    if bad.size:
        raise ValueError('g must be inside (0, 1): trace %d has %r' % (int(bad[0]), float(a[bad[0]])))
    return np.ascontiguousarray(a)


def _check_traces(y):
    """(R, T) float32 or float64, numpy or a device tensor -> (R, T, is_f64); ValueError otherwise."""
    R, T = _check_matrix(y, 'traces', ('float32', 'float64'))
    if T > MAX_FRAMES:
        raise ValueError('T = %d frames is over the limit of 2**24' % T)
    if R * T > MAX_SAMPLES:
        raise ValueError('R * T = %d samples is over the limit of 2**31' % (R * T))
    if isinstance(y, np.ndarray):
        bad = np.flatnonzero(~np.isfinite(y).all(axis=1))
        if bad.size:
            raise ValueError('traces: row %d holds a value that is not finite' % int(bad[0]))
    return R, T, str(y.dtype).endswith('float64')


class TraceDeconvolver(_MatrixStage):
    """Owns the device state of one deconvolution: the traces, the table G, the workspace of pools and the three results.  The
    kernels run at most once; result() only copies."""
    _noun = 'deconvolution'

    def __init__(self, traces, g, s_min=0.0, lam=0.0, constrain=None, sigma=None, rounds=24, device=None, baseline=0.0, baseline_rounds=8,
                 rise=None):
        """traces: (R, T) float32 or float64, numpy (checked for non-finite values) or a tensor already on the device (read in
        place, never written; THE CALLER PROMISES FINITE VALUES).  g in (0, 1): a scalar -- one decay and one table for all traces
        -- or an array of one value per trace (e.g. pick_gamma's g_each): the tables are then built on the device, one row per
        trace, and trace r gets the bits a scalar g[r] would give it.  s_min, lam: a scalar or one value per trace, >= 0.
        constrain: None, or 's_min' / 'lam': that parameter is searched per trace (it must then be left at 0) in `rounds` rounds,
        [1, 64], against sigma: None -- the noise of every trace, computed on the device where the traces lie --, a scalar or one
        value per trace (finite, >= 0, below 2**500), numpy or a float64 tensor on the device (read in place; THE CALLER PROMISES
        THAT RANGE).  baseline: one constant per trace that leaves the data inside the forward pass -- a scalar, one value per
        trace (finite), a float64 tensor on the device (read in place; THE CALLER PROMISES FINITE VALUES), or 'fit': estimated
        per trace on the device from 0, by baseline_rounds steps in [1, 64] at the given s_min and lam, or, with constrain=,
        by one step in every round of the search (baseline_rounds is then not used).  A given baseline cannot go with constrain=.
        rise: None, or the second root of the AR(2) model, a scalar with 0 < rise < g < 1 (g is then a scalar too, the decay):
        everything else works as without it, but baseline='fit' and a decay per trace are not built for AR(2)."""
        # ---- everything that can be wrong with the arguments is a ValueError before the library or the GPU is touched ----
        R, T, f64 = _check_traces(traces)
        self.rise = None
        if rise is not None:
            g, self.rise = _check_roots(g, rise)
            if isinstance(baseline, str) and baseline == 'fit':
                raise ValueError("baseline='fit' is not built for AR(2) (rise=): give the baseline or leave it out")
        self._each = np.ndim(g) != 0
        if self._each:
            self.g = _per_trace_gamma(g, R)
        else:
            self.g = _check_gamma(g)
        smin = _per_trace(s_min, 's_min', R)
        lam = _per_trace(lam, 'lam', R)
        self.constrain = constrain
        if constrain is None:
            if sigma is not None:
                raise ValueError('sigma is the noise the search is held to: it needs constrain=')
        else:
            if not isinstance(constrain, str) or constrain not in CONSTRAIN:
                raise ValueError("constrain must be None, 's_min' or 'lam', not %r" % (constrain,))
            if (smin if constrain == 's_min' else lam).any():
                raise ValueError('%s is searched (constrain=%r): it cannot also be given' % (constrain, constrain))
            self.rounds = _check_rounds(rounds, 'rounds', MAX_ROUNDS)
            if _is_device_tensor(sigma):
                _check_device_vector(sigma, 'sigma', R)
            elif sigma is not None:
                sigma = _check_sigma(sigma, R)
        self.baseline = _check_baseline(baseline, baseline_rounds, R, constrain is not None)
        self._fit = isinstance(self.baseline, str)                     # 'fit'; otherwise None or the values given
        self.baseline_rounds = int(baseline_rounds) if self._fit else None
        if self.rise is not None:
            table = ar2_table(self.g, self.rise, T)
        else:
            table = None if self._each else ar1_table(self.g, T)
        self.n_traces, self.n_frames = R, T

        self._open(device, like=traces)
        self._y, self._f64 = self._resident(traces, 'traces'), f64
        self._ld = self._row_stride(self._y, T)
        self._G = self._resident(self.g if self._each else table, 'g')         # per trace: the decays; the tables come in _decay()
        self._smin = self._resident(smin, 's_min')
        self._lam = self._resident(lam, 'lam')
        self._out = None
        self._base = None if self.baseline is None or self._fit else self._resident(self.baseline, 'the baselines')
        if constrain is not None:
            # None: the trace noise, computed in _run() and never leaving the device
            self._sigma = sigma if sigma is None else self._resident(sigma, 'the values of sigma')

    def _decay(self, stream):
        """-> (g, gs, G, ldG) as the entry points take them: one decay and one table for all traces, or the decays and one table row
        per trace, built here.  G is the tensor, not its pointer: the caller holds it until its launches are enqueued, then it goes
        back to the allocator with the workspace."""
        if not self._each:
            return self.g, None, self._G, 0
        R, T = self.n_traces, self.n_frames
        tables = self._empty((R, T + 1), 'float64')
        self.L.dc_ar1_tables(self._G.data_ptr(), R, T, tables.data_ptr(), T + 1, stream)
        return 0.0, self._G.data_ptr(), tables, T + 1

    def _run(self):
        """Everything is enqueued by one call, the whole search included: nothing is read back in between."""
        if self._out is not None:
            return self._out
        R, T, L = self.n_traces, self.n_frames, self.L
        ws_bytes = L.dc_trace_deconv_ws_bytes if self.rise is None else L.dc_trace_deconv_ar2_ws_bytes
        ws = self._empty(ws_bytes(R, T) // 8, 'float64')                       # it goes back to the allocator (stream-ordered)
        c, s, n = self._empty((R, T), 'float64'), self._empty((R, T), 'float64'), self._empty(R, 'int32')
        out = dict(calcium=c, spikes=s, pools=n)
        y, f64 = self._y.data_ptr(), int(self._f64)
        with self._torch.cuda.device(self.device):
            stream = self._stream()
            if self.constrain is not None and self._sigma is None:
                self._sigma = self._empty(R, 'float64')
                L.dc_trace_noise(y, f64, self._ld, R, T, self._sigma.data_ptr(), stream)
            g, gs, G, ldG = self._decay(stream)
            traces = (y, f64, self._ld, R, T, g, gs, G.data_ptr(), ldG)
            lam, smin = self._lam.data_ptr(), self._smin.data_ptr()
            results = (c.data_ptr(), s.data_ptr(), n.data_ptr())
            if self._fit:
                out['baseline'] = self._torch.zeros(R, dtype=self._torch.float64, device=self.device)  # b_0 = 0; the entry points write b here
                base = out['baseline'].data_ptr()
            elif self.baseline is not None:
                out['baseline'] = self._base
                base = self._base.data_ptr()
            search = self.constrain is not None
            if search:                                             # what either search takes, with a baseline to fit or without one
                state_bytes = L.dc_trace_deconv_base_state_bytes if self._fit else L.dc_trace_deconv_search_state_bytes
                state = self._empty(state_bytes(R) // 8, 'float64')
                out.update(param=self._empty(R, 'float64'), rss=self._empty(R, 'float64'), status=self._empty(R, 'int32'))
                other = self._lam if self.constrain == 's_min' else self._smin
                # what every search takes after its model: the same for AR(1) and AR(2)
                sought = (CONSTRAIN[self.constrain], self._sigma.data_ptr(), other.data_ptr(), self.rounds, ws.data_ptr(),
                          state.data_ptr()) + results + (out['param'].data_ptr(),)
                head = traces + sought
                found = (out['rss'].data_ptr(), out['status'].data_ptr())
            if self.rise is not None:                              # AR(2): one pair of roots, one table of three rows
                g1, g2 = ar2_coefficients(self.g, self.rise)
                model = (y, f64, self._ld, R, T, g1, g2, G.data_ptr(), T + 1)
                if search:
                    L.dc_trace_deconv_ar2_constrained(*model, *sought, *found, stream)
                else:
                    L.dc_trace_deconv_ar2(*model, lam, smin, None if self.baseline is None else base, ws.data_ptr(), *results, stream)
            elif search and self._fit:                             # the threshold and the baseline, jointly
                L.dc_trace_deconv_ar1_constrained_base(*head, base, *found, stream)
            elif search:
                L.dc_trace_deconv_ar1_constrained(*head, *found, stream)
            elif self._fit:                                        # the baseline at fixed parameters
                L.dc_trace_deconv_ar1_fit_base(*traces, lam, smin, self.baseline_rounds, ws.data_ptr(), *results, base, stream)
            elif self.baseline is not None:                        # a given baseline
                L.dc_trace_deconv_ar1_base(*traces, lam, smin, base, ws.data_ptr(), *results, stream)
            elif self._each:
                L.dc_trace_deconv_ar1_each(y, f64, self._ld, R, T, gs, G.data_ptr(), ldG, lam, smin, ws.data_ptr(), *results, stream)
            else:
                L.dc_trace_deconv_ar1(y, f64, self._ld, R, T, g, G.data_ptr(), lam, smin, ws.data_ptr(), *results, stream)
            if search:
                out['target'] = state[3 * R:4 * R].clone()         # plane 3 of the state holds the targets
        self._out = out
        return out

    @property
    def sigma_device(self):
        """The noise a constrained object was held to, float64[R] on the device (computed there when none was given)."""
        if self.constrain is None:
            raise ValueError('an unconstrained deconvolution has no sigma')
        self._run()
        return self._sigma

    def result_device(self, kind='spikes'):
        """result(kind) as a tensor on the device (the object's own state: do not write to it): (R, T) float64 for 'calcium' and
        'spikes', int32[R] for 'pools'; of a constrained object also float64[R] for 'param', 'rss' and 'target' and int32[R] for
        'status'; float64[R] for 'baseline', the constants taken off the traces (zeros where none was asked for)."""
        if kind == 'baseline':
            out = self._run()
            if 'baseline' not in out:
                with self._torch.cuda.device(self.device):
                    out['baseline'] = self._torch.zeros(self.n_traces, dtype=self._torch.float64, device=self.device)
            return out['baseline']
        _check_kind(kind, self.constrain is not None)
        return self._run()[kind]


def deconvolve_traces_device(dspath, rois, window, tau, fps=None, k=3.0, lam=0.0, details=False, lags=5, g_min=0.05, g_max=0.998, baseline=0.0,
                             tau_rise=None, rise_lags=10, **dff_kw):
    """-> (calcium, spikes), float64 (R, T): the dF/F traces of `rois` over a dataset file (dff_traces_device(dspath, rois, window,
    **dff_kw)) deconvolved with s_min = k * sigma_hat per trace and the penalty lam.  tau: a number -- the decay time in seconds,
    g = ar1_gamma(tau, fps) --, 'auto' -- the decay is estimated per trace from the dF/F (deep_calcium_amd.dynamics: TraceDynamics
    with `lags`, then pick_gamma with g_min, g_max) and the pooled median serves all traces --, or 'each' -- every trace is
    deconvolved with its own estimate.  fps is needed for a number only.  details=True -> (calcium, spikes, info), info =
    dict(g=the decay used, a float or float64[R] for 'each'; g_raw=, status=, pooled= what pick_gamma gave, None for a number;
    sigma=sigma_hat float64[R]).  k='noise': no k at all -- s_min is searched per trace so that the residual stays within the
    noise (TraceDeconvolver(constrain='s_min'), held to the same sigma_hat, which stays on the device); info then also has
    s_min= the thresholds found, rss= their residuals and search_status= (0 bracketed, 1 s_min = 0, 2 never bracketed).
    baseline: TraceDeconvolver's -- a scalar, or 'fit': one constant per trace estimated on the device; info['baseline'] is
    float64[R], the values used.  Recommended: k='noise' with baseline='fit' -- dF/F over a low percentile sits about one sigma
    above zero when the cell is quiet, which the search alone pays for with spurious events.  With a numeric k the fit is only as
    good as the threshold (one that is too high lets missed events lift the baseline).  tau_rise: the rise time in seconds of an
    AR(2) model, rise = ar1_gamma(tau_rise, fps) (TraceDeconvolver(rise=)); it needs a numeric tau above it, and baseline='fit' is
    not built for it; info then also has rise=.  tau='auto' with tau_rise='auto': both roots are estimated from the dF/F
    (deep_calcium_amd.dynamics: TraceDynamicsAR2 with `rise_lags`, then pick_roots with d_max = g_max) and the pooled pair serves
    all traces; info then has g= and rise= the pooled roots, pooled=(g, rise), g12_raw=, root_status= what pick_roots gave, and
    g_raw= the AR(1) estimates at these lags (status= is None).  With no trace of two usable roots it is a ValueError: give tau
    and tau_rise."""
    mode = tau if isinstance(tau, str) else None
    if mode is not None and mode not in ('auto', 'each'):
        raise ValueError("tau must be a number of seconds, 'auto' or 'each', not %r" % (tau,))
    rise, rise_auto = None, False
    if isinstance(tau_rise, str):                                    # both roots estimated: the decay and the rise, pooled
        if tau_rise != 'auto':
            raise ValueError("tau_rise must be a number of seconds or 'auto', not %r" % (tau_rise,))
        if mode != 'auto':
            raise ValueError("tau_rise='auto' estimates both roots, pooled over the traces: it needs tau='auto', not tau=%r (a given "
                             'decay beside an estimated rise, and roots per trace, are not built)' % (tau,))
        if isinstance(baseline, str) and baseline == 'fit':
            raise ValueError("baseline='fit' is not built for AR(2) (tau_rise=)")
        from .dynamics import _check_lags
        try:
            _check_lags(rise_lags, 2)
        except ValueError as e:
            raise ValueError('rise_%s' % e)
        rise_auto = True
    elif tau_rise is not None:
        if mode is not None:
            raise ValueError('tau_rise needs a number of seconds for tau: estimating the decay (tau=%r) is not built for AR(2)' % (tau,))
        if isinstance(baseline, str) and baseline == 'fit':
            raise ValueError("baseline='fit' is not built for AR(2) (tau_rise=)")
        rise = _check_roots(ar1_gamma(tau, fps), ar1_gamma(tau_rise, fps))[1]
    if mode is None:
        g = ar1_gamma(tau, fps)
    else:
        from .dynamics import _check_lags, pick_gamma
        _check_lags(lags)
        pick_gamma(np.array([0.5]), g_min, g_max)                    # the bounds, before anything is opened
        if fps is not None:
            ar1_gamma(1.0, fps)
    search = isinstance(k, str)
    if search:
        if k != 'noise':
            raise ValueError("k must be a number >= 0 or 'noise', not %r" % (k,))
    else:
        try:
            k = float(k)
        except (TypeError, ValueError):
            raise ValueError('k must be a number >= 0, not %r' % (k,))
        if not 0.0 <= k < np.inf:
            raise ValueError('k must be finite and >= 0, not %r' % (k,))
    if np.ndim(lam) != 0:
        raise ValueError('lam must be a scalar here, not shape %r' % (np.shape(lam),))
    _per_trace(lam, 'lam', 1)
    if not isinstance(baseline, str) and (_is_device_tensor(baseline) or np.ndim(baseline) != 0):
        raise ValueError("baseline must be a scalar or 'fit' here, not %s" % type(baseline).__name__)
    with_base = _check_baseline(baseline, 8, 1, search) is not None
    if dff_kw.get('kind', 'dff') != 'dff':
        raise ValueError('the deconvolution takes dF/F: kind = %r is not supported' % (dff_kw['kind'],))
    from .dff import dff_traces_device
    dff = dff_traces_device(dspath, rois, window, **dff_kw)
    if mode is None:
        if search:
            dec = TraceDeconvolver(dff, g, lam=lam, constrain='s_min', device=dff_kw.get('device'), baseline=baseline, rise=rise)
            sigma = dec.sigma_device.cpu().numpy()
        else:
            sigma = trace_noise(dff)
            dec = TraceDeconvolver(dff, g, s_min=k * sigma, lam=lam, device=dff_kw.get('device'), baseline=baseline, rise=rise)
        info = dict(g=g, g_raw=None, status=None, sigma=sigma, pooled=None)
        if rise is not None:
            info['rise'] = rise
    elif rise_auto:
        from .dynamics import TraceDynamicsAR2, pick_roots
        dyn = TraceDynamicsAR2(dff, lags=rise_lags, device=dff_kw.get('device'))
        sigma, g12_raw = dyn.result('noise'), dyn.result('g12_raw')
        _, root_status, (g, rise) = pick_roots(g12_raw, d_max=g_max)
        if search:
            dec = TraceDeconvolver(dyn.traces_device, g, lam=lam, constrain='s_min', sigma=dyn.result_device('noise'), device=dyn.device,
                                   baseline=baseline, rise=rise)
        else:
            dec = TraceDeconvolver(dyn.traces_device, g, s_min=k * sigma, lam=lam, device=dyn.device, baseline=baseline, rise=rise)
        info = dict(g=g, rise=rise, g_raw=dyn.result('g_raw'), status=None, sigma=sigma, pooled=(g, rise), g12_raw=g12_raw,
                    root_status=root_status)
    else:
        from .dynamics import TraceDynamics
        dyn = TraceDynamics(dff, lags=lags, device=dff_kw.get('device'))
        sigma, g_raw = dyn.result('noise'), dyn.result('g_raw')
        g_each, status, g_pool = pick_gamma(g_raw, g_min, g_max)
        g = g_pool if mode == 'auto' else g_each
        if search:
            dec = TraceDeconvolver(dyn.traces_device, g, lam=lam, constrain='s_min', sigma=dyn.result_device('noise'), device=dyn.device,
                                   baseline=baseline)
        else:
            dec = TraceDeconvolver(dyn.traces_device, g, s_min=k * sigma, lam=lam, device=dyn.device, baseline=baseline)
        info = dict(g=g, g_raw=g_raw, status=status, sigma=sigma, pooled=g_pool)
    if with_base:
        info['baseline'] = dec.result('baseline')
    if search:
        info.update(s_min=dec.result('param'), rss=dec.result('rss'), search_status=dec.result('status'))
    if details:
        return dec.result('calcium'), dec.result('spikes'), info
    return dec.result('calcium'), dec.result('spikes')
