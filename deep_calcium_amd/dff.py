"""dF/F traces on the device: neuropil correction, a rolling-percentile baseline F0(t) and (F - F0) / F0.

The step between ROI traces (deep_calcium_amd/traces.py) and spikes that a z-score over the whole recording cannot replace: a
recording bleaches and drifts over minutes, and every ROI collects out-of-focus neuropil light.  The reference has no counterpart;
the definitions in include/dcunet.h ("dF/F traces") are the specification.  From the int64 ROI sums S and areas A the
dc_trace_* kernels form

    kind          dtype     what
    num           int64     N = S + o A, or with a neuropil ring (An pixels, sums Sn, weight a / 256):
                            N = 256 An (S + o A) - a A (Sn + o An)                                     (exact)
    baseline_sum  int64     B_t = the k-th smallest of N over frames [t - h, t + h] clipped to the trace,
                            k = (q * (n - 1)) // 100                                                   (exact)
    f             float32   N / D, D = A or 256 An A: the corrected fluorescence per pixel             (bit-equal to numpy's float64 divide)
    baseline      float32   B / D                                                                      (bit-equal)
    dff           float32   (N - B) / B where B > 0, else 0                                            (bit-equal)

    rings = neuropil_rois(rois, (H, W), inner=2, outer=12)
    tb = TraceBaseline(sums, areas, window=1801, percentile=8, neuropil_sums=ring_sums, neuropil_areas=ring_areas, weight=0.7)
    dff = tb.result('dff')                        # (R, T)

    dff = dff_traces_device('dataset.hdf5', mask, window=1801, neuropil=(2, 12, 0.7))     # one streaming pass, then the kernels

The rank is an integer rule, not numpy's float one (floor(0.29 * 100) is 28): compare with np.sort(window)[k], never np.percentile.

Importing this module needs neither torch nor the GPU; constructing a TraceBaseline does (there is no CPU fallback).
"""
import numpy as np

from ._matrix import _MatrixStage, _check_matrix, _is_device_tensor                # noqa: F401 (the last: importable from here as before)
from ._reader import _read_recording
from .traces import RoiTraceExtractor, _check_shape, _roi_pixels

KINDS = ('num', 'baseline_sum', 'f', 'baseline', 'dff')
MAX_HALF = 2047                       # DC_TRACE_BASELINE_MAX_HALF: the longest window is 4095 frames
MAX_OFFSET = 65535
MAX_RING = 64                         # neuropil_rois: the largest outer distance
MAX_AREA_PRODUCT = 1 << 36            # An * A below this keeps |N| < 2**62


def _check_kind(kind):
    if kind not in KINDS:
        raise ValueError('dF/F kind %r is not one of %s' % (kind, ', '.join(KINDS)))


def _as_int(v, what):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError('%s must be an integer, not %r' % (what, v))
    return int(v)


def window_half(window):
    """The half-width h of an odd window of 2h + 1 frames."""
    window = _as_int(window, 'window')
    if window < 1 or window % 2 == 0:
        raise ValueError('window must be an odd, positive number of frames (2h + 1), not %d' % window)
    if window // 2 > MAX_HALF:
        raise ValueError('window = %d frames is over the limit of %d' % (window, 2 * MAX_HALF + 1))
    return window // 2


def _check_percentile(q):
    q = _as_int(q, 'percentile')
    if not 0 <= q <= 100:
        raise ValueError('percentile must be an integer in [0, 100], not %d' % q)
    return q


def _check_offset(o):
    o = _as_int(o, 'offset')
    if abs(o) > MAX_OFFSET:
        raise ValueError('offset must be within +-%d, not %d' % (MAX_OFFSET, o))
    return o


def rank_index(q, n):
    """k = (q * (n - 1)) // 100: the 0-based rank of integer percentile q among n samples (dc_dff_rank of csrc/dff_math.h)."""
    return (int(q) * (int(n) - 1)) // 100


def weight_256ths(weight):
    """a = floor(256 w + 0.5) for a neuropil weight w in [0, 1]."""
    try:
        w = float(weight)
    except (TypeError, ValueError):
        raise ValueError('weight must be a number in [0, 1], not %r' % (weight,))
    if not 0.0 <= w <= 1.0:                     # NaN fails both comparisons
        raise ValueError('weight must be in [0, 1], not %r' % (weight,))
    return int(np.floor(256.0 * w + 0.5))


def _check_areas(areas, what, R=None, zero_ok=False):
    a = np.asarray(areas)
    if a.ndim != 1 or a.dtype.kind not in 'iu' or (R is not None and a.shape[0] != R):
        raise ValueError('%s must be an integer vector%s, not %s %r' % (what, '' if R is None else ' of %d' % R, a.dtype, a.shape))
    a = a.astype(np.int64)
    if a.size and (a.min() < (0 if zero_ok else 1) or a.max() > (1 << 30)):
        raise ValueError('%s must be in [%d, 2**30]' % (what, 0 if zero_ok else 1))
    return a


def combine_coefficients(areas, neuropil_areas=None, weight=0.7, offset=0):
    """-> (ca, cb, cc, den, corrected): int64[R] each and a bool[R].  With S the ROI's sums and Sn its ring's,
    N = ca * S - cb * Sn + cc and D = den (include/dcunet.h): without neuropil or where neuropil_areas[r] == 0, ca = 1, cb = 0,
    cc = o A, D = A; otherwise ca = 256 An, cb = a A, cc = o A An (256 - a), D = 256 An A.  An * A >= 2**36 is a ValueError
    naming the ROI: below it |N| < 2**62 for sums of 16-bit pixels."""
    A = _check_areas(areas, 'areas')
    o = _check_offset(offset)
    a = weight_256ths(weight)
    R = len(A)
    An = np.zeros(R, np.int64) if neuropil_areas is None else _check_areas(neuropil_areas, 'neuropil_areas', R, zero_ok=True)
    # An, A <= 2**30: the product fits int64
    over = np.flatnonzero(An * A >= MAX_AREA_PRODUCT)
    if over.size:
        r = int(over[0])
        raise ValueError('ROI %d: area %d times neuropil area %d is not below 2**36' % (r, A[r], An[r]))
    on = An > 0
    ca = np.where(on, 256 * An, 1)
    cb = np.where(on, a * A, 0)
    cc = np.where(on, o * A * An * (256 - a), o * A)
    den = np.where(on, 256 * An * A, A)
    return ca.astype(np.int64), cb.astype(np.int64), cc.astype(np.int64), den.astype(np.int64), on


# ---- the neuropil rings ----------------------------------------------------------------------------------------------------
def _dilate(m, r):
    """Every pixel within Chebyshev distance r of a set pixel: the square (2r + 1)-dilation, separable, from shifted copies."""
    out = m.copy()
    for d in range(1, r + 1):
        out[d:] |= m[:-d]
        out[:-d] |= m[d:]
    m = out
    out = m.copy()
    for d in range(1, r + 1):
        out[:, d:] |= m[:, :-d]
        out[:, :-d] |= m[:, d:]
    return out


def _rings(pixels, shape, inner, outer):
    H, W = shape
    every = np.zeros((H, W), bool)
    for p in pixels:
        every.ravel()[p] = True
    near = _dilate(every, inner)                 # within `inner` of ANY ROI (the ROIs' own pixels included): in no ring
    out = []
    for p in pixels:
        y, x = p // W, p % W
        y0, y1 = max(0, int(y.min()) - outer), min(H, int(y.max()) + outer + 1)      # the ring cannot leave this box
        x0, x1 = max(0, int(x.min()) - outer), min(W, int(x.max()) + outer + 1)
        own = np.zeros((y1 - y0, x1 - x0), bool)
        own[y - y0, x - x0] = True
        ring = _dilate(own, outer) & ~near[y0:y1, x0:x1]
        c = np.argwhere(ring)                    # raster order
        out.append((c + np.array([y0, x0])).astype(np.int64).reshape(-1, 2))
    return out


def _check_ring(inner, outer):
    inner, outer = _as_int(inner, 'inner'), _as_int(outer, 'outer')
    if not 0 <= inner < outer <= MAX_RING:
        raise ValueError('the ring needs 0 <= inner < outer <= %d, not inner = %d, outer = %d' % (MAX_RING, inner, outer))
    return inner, outer


def neuropil_rois(rois, shape, inner=2, outer=12):
    """One neuropil ring per ROI: a (k, 2) int64 array of [y, x] in raster order, possibly empty.  With the Chebyshev distance d,
    the ring of ROI r holds the pixels p with inner < d(p, ROI r) <= outer that are not within `inner` of ANY ROI (the ROIs' own
    pixels included), so that no ring collects a neighbour's light.  `rois`: every form rois_to_csr takes.  Host numpy only."""
    shape = _check_shape(shape)
    inner, outer = _check_ring(inner, outer)
    return _rings(_roi_pixels(rois, shape), shape, inner, outer)


# ---- the device state ---------------------------------------------------------------------------------------------------------
def _check_sums(x, what, shape=None):
    """(R, T) int64, numpy or a device tensor -> its shape; ValueError otherwise."""
    return _check_matrix(x, what, ('int64',), shape)


class TraceBaseline(_MatrixStage):
    """Owns the device state of one recording's dF/F: the numerators N, their rolling-percentile baseline B and the float
    results.  Every kernel runs at most once; result() only copies."""
    _noun = 'baseline'

    def __init__(self, sums, areas, window, percentile=8, offset=0, neuropil_sums=None, neuropil_areas=None, weight=0.7, device=None):
        """sums: (R, T) int64, numpy or a tensor already on the device (read in place).  areas: the R pixel counts.  window: the
        odd number of frames 2h + 1.  neuropil_sums / neuropil_areas: the (R, T) sums and the R pixel counts of the ROIs'
        neuropil rings, row for row; neuropil_areas[r] == 0 means no correction for ROI r (its row of neuropil_sums is ignored)."""
        # ---- everything that can be wrong with the arguments is a ValueError before the library or the GPU is touched ----
        R, T = _check_sums(sums, 'sums')
        if (neuropil_sums is None) != (neuropil_areas is None):
            raise ValueError('give neuropil_sums and neuropil_areas together, or neither')
        if neuropil_sums is not None:
            _check_sums(neuropil_sums, 'neuropil_sums', (R, T))
        areas = _check_areas(areas, 'areas', R)
        coeff = combine_coefficients(areas, neuropil_areas, weight, offset)
        np_row = np.where(coeff[4], R + np.arange(R), -1).astype(np.int32)
        self._setup(sums, neuropil_sums, R, T, np_row, coeff, window, percentile, device)

    @classmethod
    def from_stacked(cls, sums, areas, ring_rows, ring_areas, window, percentile=8, offset=0, weight=0.7, device=None):
        """One matrix holds both: rows [0, R) of `sums` are the ROIs (R = len(areas)), and ring_rows[r] names the row that holds
        the neuropil ring of ROI r (ring_areas[r] pixels), or is negative for an ROI without one -- what one streaming pass over
        the ROIs followed by their non-empty rings leaves behind (dff_traces_device).  Nothing is copied."""
        rows, T = _check_sums(sums, 'sums')
        areas = _check_areas(areas, 'areas')
        R = len(areas)
        ring_rows = np.asarray(ring_rows)
        if ring_rows.shape != (R,) or ring_rows.dtype.kind not in 'iu' or R > rows or (ring_rows.size and ring_rows.max() >= rows):
            raise ValueError('ring_rows must name, for each of the %d ROIs, one of the %d rows of sums (or be negative)' % (R, rows))
        ring_areas = np.where(ring_rows >= 0, _check_areas(ring_areas, 'ring_areas', R, zero_ok=True), 0)
        if ((ring_rows >= 0) & (ring_areas == 0)).any():
            raise ValueError('a ring that has a row of sums cannot have area 0')
        coeff = combine_coefficients(areas, ring_areas, weight, offset)
        np_row = np.where(coeff[4], ring_rows, -1).astype(np.int32)
        self = cls.__new__(cls)
        self._setup(sums, None, R, T, np_row, coeff, window, percentile, device)
        return self

    def _setup(self, sums, neuropil_sums, R, T, np_row, coeff, window, percentile, device):
        self.half = window_half(window)
        self.percentile = _check_percentile(percentile)
        self.n_rois, self.n_frames = R, T
        self._den_host = coeff[3]

        torch = self._open(device, like=sums)
        dev = self.device
        src = self._resident(sums, 'sums')
        if neuropil_sums is not None and (np_row >= 0).any():
            src = torch.cat([src, self._resident(neuropil_sums, 'neuropil_sums')], 0)       # one matrix: np_row names rows >= R
        self._src = src
        self._ld = self._row_stride(src, T)
        self._np_row = torch.from_numpy(np_row).to(dev)
        self._ca, self._cb, self._cc, self._den = [torch.from_numpy(c).to(dev) for c in coeff[:4]]
        self._num = self._base = self._dff = None

    def _numerators(self):
        if self._num is None:
            R, T = self.n_rois, self.n_frames
            num = self._empty((R, T), 'int64')
            with self._torch.cuda.device(self.device):
                self.L.dc_trace_combine(self._src.data_ptr(), self._ld, self._np_row.data_ptr(), self._ca.data_ptr(), self._cb.data_ptr(),
                                        self._cc.data_ptr(), R, T, num.data_ptr(), self._stream())
            self._num = num
        return self._num

    def _baseline(self):
        if self._base is None:
            R, T = self.n_rois, self.n_frames
            num = self._numerators()
            base, dff = self._empty((R, T), 'int64'), self._empty((R, T), 'float32')
            with self._torch.cuda.device(self.device):
                self.L.dc_trace_baseline(num.data_ptr(), T, R, T, self.half, self.percentile, base.data_ptr(), dff.data_ptr(),
                                         self._stream())
            self._base, self._dff = base, dff
        return self._base, self._dff

    def _scaled(self, x):
        R, T = self.n_rois, self.n_frames
        out = self._empty((R, T), 'float32')
        with self._torch.cuda.device(self.device):
            self.L.dc_trace_scale(x.data_ptr(), T, self._den.data_ptr(), R, T, out.data_ptr(), self._stream())
        return out

    def denominators(self):
        """D, int64[R]: A, or 256 An A for an ROI with a neuropil ring."""
        return self._den_host.copy()

    def result_device(self, kind='dff'):
        """result(kind) as a tensor on the device (int64 results are the object's own state: do not write to them): (R, T), int64
        for 'num' and 'baseline_sum', float32 for 'f', 'baseline' and 'dff'."""
        _check_kind(kind)
        if kind == 'num':
            return self._numerators()
        if kind == 'f':
            return self._scaled(self._numerators())
        base, dff = self._baseline()
        return base if kind == 'baseline_sum' else dff if kind == 'dff' else self._scaled(base)


def dff_traces_device(dspath, rois, window, percentile=8, kind='dff', neuropil=None, offset=0, source='series/raw', device=None,
                      chunk_frames=None, weights=None, shifts=None, fine_shifts=None, bidi=0):
    """The (R, T) dF/F traces (or any other kind of KINDS) of `rois` over `source` of a dataset file.  neuropil: None, or
    (inner, outer, weight): every ROI is corrected by its ring neuropil_rois(rois, shape, inner, outer).  The recording is read
    ONCE, by a single RoiTraceExtractor whose ROI list is the ROIs followed by the non-empty rings; combine, baseline and scale
    then run on the sums where they lie.  shifts / fine_shifts / bidi: as for extract_traces_device.
    weights: None, or one integer array per ROI (weighted.WeightedTraceExtractor; rois is then a list of (k,2) arrays or region dicts):
    the ROI sums are the weighted ones and the weight sum W_r stands where the area stood.  The rings stay unweighted."""
    _check_kind(kind)
    window_half(window)
    _check_percentile(percentile)
    _check_offset(offset)
    weight = 0.0
    if neuropil is not None:
        try:
            inner, outer, weight = neuropil
        except (TypeError, ValueError):
            raise ValueError('neuropil must be None or (inner, outer, weight), not %r' % (neuropil,))
        inner, outer = _check_ring(inner, outer)
        weight_256ths(weight)
    stacked = []

    def reader_of(shape, T, dtype, **kw):
        """One extractor whose ROI list is the ROIs followed by the non-empty rings, built from the shape before the pass."""
        shape = _check_shape(shape)
        if weights is not None:
            from .weighted import _check_wsums, _weighted_entries
            entries = _weighted_entries(rois, weights, shape)
            pixels = [f.astype(np.int32) for f, _ in entries]
            areas = _check_wsums(entries, T)                             # W_r
        else:
            pixels = _roi_pixels(rois, shape)
            areas = np.array([len(p) for p in pixels], np.int64)
        R = len(pixels)
        ring_rows, ring_areas = np.full(R, -1, np.int64), np.zeros(R, np.int64)
        every = [np.stack([p // shape[1], p % shape[1]], 1) for p in pixels]
        if neuropil is not None:
            for r, ring in enumerate(_rings(pixels, shape, inner, outer)):
                if len(ring):
                    ring_rows[r], ring_areas[r] = len(every), len(ring)
                    every.append(ring)
        combine_coefficients(areas, ring_areas, weight, offset)          # An * A over the limit: before the pass, not after it
        stacked.extend((areas, ring_rows, ring_areas))
        if weights is None:
            return RoiTraceExtractor(shape, T, dtype, every, **kw)
        from .weighted import WeightedTraceExtractor                     # one weighted pass: a ring pixel has weight 1
        return WeightedTraceExtractor(shape, T, dtype, every, [w for _, w in entries] + [np.ones(len(c), np.int64) for c in every[R:]], **kw)
    ext = _read_recording(dspath, source, reader_of, device, chunk_frames, shifts, fine_shifts, bidi)
    areas, ring_rows, ring_areas = stacked
    return TraceBaseline.from_stacked(ext.sums_device(), areas, ring_rows, ring_areas, window, percentile=percentile, offset=offset,
                                      weight=weight, device=ext.device).result(kind)
