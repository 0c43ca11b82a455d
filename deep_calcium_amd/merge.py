"""Merging fragmented ROIs: the correlation over time of the traces of neighbouring ROIs, and the union of those that move together.

A mask predicted from ONE summary image makes three kinds of mistakes.  refine_rois (footprints.py) drops pixels and structures
that never fire, split_rois (roi_pairs.py) cuts an ROI that holds two cells; this module handles the opposite case, ONE cell that
arrives as SEVERAL ROIs -- a nucleus-excluded ring broken into arcs, a cell cut by a one-pixel line of sub-threshold probability,
an over-eager split.  Each fragment would get its own trace, dF/F and spike train, and the cell would be counted twice.  The
reference has no counterpart; the definitions in include/dcunet.h ("ROI trace-pair correlation") are the specification.

What decides a merge is the correlation over time of the traces of two neighbouring ROIs.  Its inputs already lie on the device
after the streaming pass -- the int64 (R, T) sums of RoiTraceExtractor.sums_device() -- so no further pass over the recording is
needed:

    kind        dtype     what
    moments     int       Nxx, Nxy, Nyy of every candidate pair: exact 128-bit integers                 (exact)
    corr        float32   corr(trace_i, trace_j), one value per pair                                     (exact numerators, <= 1 ulp)

    pairs = roi_neighbours(rois, (H, W), max_dist=2)                  # host: which ROIs lie within 2 pixels of each other
    ext = RoiTraceExtractor((H, W), T, np.int16, rois); ...feed...    # the one streaming pass
    tp = TracePairCorr(ext.sums_device(), ext.areas_host(), pairs, detrend_frames=128)
    new_rois, origin = merge_rois(pixels, pairs, tp.result('corr'), (H, W), threshold=0.8)

    new_rois, origin, pairs, corr = merge_rois_device('dataset.hdf5', mask, detrend_frames=128)      # one call, one pass

Bleaching pushes EVERY trace pair towards 1: on the two-cell scene of the tests at T = 1024, a decay to half the brightness lifts
the correlation of the two DISTINCT cells from -0.10 .. 0.27 to 0.895 .. 0.949, and any sensible threshold merges all 40 pairs.
detrend_frames=L correlates within segments of L frames and pools them (series.detrend_plan): at L = 128 they are back at
0.005 .. 0.446 while the two halves of one cell stay at 0.933 .. 0.968.  Use it on every recording that bleaches or drifts.

The merge rule (merge_rois; host, deterministic): the candidate pairs with corr >= threshold are the edges of a graph on the
ROIs; every connected component becomes one ROI, the sorted, de-duplicated union of its members' pixels.  SINGLE LINKAGE: A-B and
B-C merge A with C whatever corr(A, C) is.  One round per call: a merged ROI has a new trace, and merging further is another
call.  The threshold is a definition, not a measurement; 0.8 is the value CaImAn ships.

Importing this module needs neither torch nor the GPU; constructing a TracePairCorr does (there is no CPU fallback).
"""
import numpy as np

from ._matrix import _MatrixStage
from .dff import _as_int, _check_areas, _check_sums, _dilate
from .footprints import MAX_FRAMES
from .traces import MAX_VOLUME, _check_shape, _roi_pixels

KINDS = ('moments', 'corr')
MAX_DIST = 16                         # roi_neighbours: the largest Chebyshev distance
MAX_PAIRS = 1 << 24                   # DC_TRACE_PAIR_MAX_PAIRS


def _check_kind(kind):
    if kind not in KINDS:
        raise ValueError('trace-pair kind %r is not one of %s' % (kind, ', '.join(KINDS)))


def _check_max_dist(max_dist):
    max_dist = _as_int(max_dist, 'max_dist')
    if not 0 <= max_dist <= MAX_DIST:
        raise ValueError('max_dist must be in [0, %d], not %d' % (MAX_DIST, max_dist))
    return max_dist


def _check_threshold(threshold):
    if isinstance(threshold, (bool, np.bool_)):
        raise ValueError('threshold must be a number, not %r' % (threshold,))
    try:
        threshold = float(threshold)
    except (TypeError, ValueError):
        raise ValueError('threshold must be a number, not %r' % (threshold,))
    if threshold != threshold:
        raise ValueError('threshold must be a number, not NaN')
    return threshold


def _check_pairs(pairs, R):
    """-> int32 (P, 2), C-contiguous; ValueError for anything that is not a list of pairs of ROI indices in [0, R)."""
    p = np.asarray(pairs)
    if p.ndim == 1 and p.size == 0:
        p = p.reshape(0, 2).astype(np.int32)
    if p.ndim != 2 or p.shape[1] != 2 or p.dtype.kind not in 'iu':
        raise ValueError('pairs must be a (P, 2) integer array of ROI indices, not %s %r' % (p.dtype, p.shape))
    if len(p) > MAX_PAIRS:
        raise ValueError('%d pairs: limited to 2**24 = %d' % (len(p), MAX_PAIRS))
    if p.size and (int(p.min()) < 0 or int(p.max()) >= R):
        bad = int(np.flatnonzero(((p < 0) | (p >= R)).any(1))[0])
        raise ValueError('pair %d = (%d, %d) names an ROI outside [0, %d)' % (bad, int(p[bad, 0]), int(p[bad, 1]), R))
    return np.ascontiguousarray(p.astype(np.int32))


def _coords(flat, W):
    flat = flat.astype(np.int64)
    return np.stack([flat // W, flat % W], 1)


def roi_neighbours(rois, shape, max_dist=2):
    """-> int32 (P, 2): the pairs (i, j), i < j, in lexicographic order, of ROIs whose pixel sets lie within Chebyshev distance
    max_dist of each other: 0 -- they share a pixel; 1 -- they also may merely touch (8-neighbours); 2 -- one blank pixel between.
    max_dist in [0, 16].  `rois`: every form rois_to_csr takes.  Host numpy only."""
    shape = _check_shape(shape)
    max_dist = _check_max_dist(max_dist)
    H, W = shape
    pixels = _roi_pixels(rois, shape)
    every = np.concatenate(pixels).astype(np.int64)
    owner = np.repeat(np.arange(len(pixels)), [len(p) for p in pixels])
    order = np.argsort(every, kind='stable')
    every, owner = every[order], owner[order]
    out = []
    for i, p in enumerate(pixels):
        p = p.astype(np.int64)
        y, x = p // W, p % W
        y0, y1 = max(0, int(y.min()) - max_dist), min(H, int(y.max()) + max_dist + 1)      # the dilation cannot leave this box
        x0, x1 = max(0, int(x.min()) - max_dist), min(W, int(x.max()) + max_dist + 1)
        own = np.zeros((y1 - y0, x1 - x0), bool)
        own[y - y0, x - x0] = True
        c = np.argwhere(_dilate(own, max_dist))
        near = (c[:, 0] + y0) * W + (c[:, 1] + x0)
        js = np.unique(owner[np.isin(every, near)])
        out += [(i, int(j)) for j in js if j > i]
    return np.array(out, np.int32).reshape(-1, 2)


def _check_range(T, areas, detrend_frames):
    """-> (seg_len, M) of T frames under detrend_frames (0, T for None); ValueError where L is out of range, T > 2**31 - 1, or an
    ROI's area takes the sums out of the range of the 128-bit numerators: max(M, T) * area > 2**46."""
    if T > MAX_FRAMES:
        raise ValueError('the sums have %d frames: limited to 2**31 - 1' % T)
    L, M = 0, T
    if detrend_frames is not None:
        from .series import _check_detrend_frames, detrend_plan
        L = _check_detrend_frames(detrend_frames)
        plan = detrend_plan(T, L)
        M = plan[0][1] * plan[0][2]
    worst = int(np.argmax(areas))
    if max(M, T) * int(areas[worst]) > MAX_VOLUME:
        raise ValueError('ROI %d has %d pixels: max(M, T) * area = %d * %d is limited to 2**46' % (worst, int(areas[worst]), max(M, T),
                                                                                               int(areas[worst])))
    return L, M


class TracePairCorr(_MatrixStage):
    """Owns the device state of the trace-pair correlation of one list of candidate pairs.  Every kernel runs at most once;
    result() only copies."""
    _noun = 'pair correlation'

    def __init__(self, sums, areas, pairs, detrend_frames=None, device=None):
        """sums: (R, T) int64, numpy or a tensor already on the device (read in place: RoiTraceExtractor.sums_device()).  areas: the R
        pixel counts (RoiTraceExtractor.areas_host()): they bound the sums, |S| <= 2**16 * area.  pairs: (P, 2) integers, any
        order, i == j allowed, a pair may appear twice.  detrend_frames: None, or an integer L in [2, 4096]: the numerators are
        pooled over the segments of series.detrend_plan(T, L); L > T / 2 is one segment: the bits of None.
        ValueError before the GPU is touched: bad pairs or an index outside [0, R), L out of range, T > 2**31 - 1, and
        max(M, T) * max(areas) > 2**46 (M = L * L_last of the plan), naming the ROI: beyond it the 128-bit numerators may not fit."""
        # ---- everything that can be wrong with the arguments is a ValueError before the library or the GPU is touched ----
        R, T = _check_sums(sums, 'sums')
        areas = _check_areas(areas, 'areas', R)
        pairs = _check_pairs(pairs, R)
        L, M = _check_range(T, areas, detrend_frames)
        self.n_rois, self.n_frames, self.n_pairs = R, T, len(pairs)
        self.seg_len, self.M = L, M
        self._pairs_host = pairs

        torch = self._open(device, like=sums)
        self._src = self._resident(sums, 'sums')
        self._ld = self._row_stride(self._src, T)
        self._pairs = torch.from_numpy(pairs).to(self.device)
        self._num = self._corr = None

    def pairs(self):
        """The (P, 2) int32 pairs, in the order of the results."""
        return self._pairs_host.copy()

    def _numerators(self):
        if self._num is None:
            num = self._empty((self.n_pairs, 6), 'int64')
            with self._torch.cuda.device(self.device):
                if self.n_pairs:
                    self.L.dc_trace_pair_moments(self._src.data_ptr(), self._ld, self.n_rois, self.n_frames, self.seg_len,
                                                 self._pairs.data_ptr(), self.n_pairs, num.data_ptr(), self._stream())
            self._num = num
        return self._num

    def result_device(self, kind='corr'):
        """result(kind) as a tensor on the device: 'corr' float32 (P,); 'moments' the int64 (P, 6) words {Nxx, Nxy, Nyy} x {lo, hi}
        (the object's own state: do not write to them)."""
        _check_kind(kind)
        num = self._numerators()
        if kind == 'moments':
            return num
        if self._corr is None:
            corr = self._empty((self.n_pairs,), 'float32')
            with self._torch.cuda.device(self.device):
                if self.n_pairs:
                    self.L.dc_trace_pair_corr(num.data_ptr(), self.n_pairs, corr.data_ptr(), self._stream())
            self._corr = corr
        return self._corr

    def result(self, kind='corr'):
        """'corr': float32 (P,), one value per pair; 'moments': a list of P dict(Nxx, Nxy, Nyy, M) of exact Python ints -- the
        numerators before any float, and the M of the plan (T for one segment)."""
        _check_kind(kind)
        if kind == 'corr':
            return self.result_device('corr').cpu().numpy()
        from .series import _pooled_ints
        words = _pooled_ints(self._numerators().cpu().numpy().reshape(self.n_pairs, 3, 2))
        return [dict(Nxx=int(w[0]), Nxy=int(w[1]), Nyy=int(w[2]), M=self.M) for w in words]


def merge_rois(pixels, pairs, corr, shape, threshold=0.8):
    """-> (new_rois, origin).  pixels: per ROI a (k, 2) integer array of [y, x] (every list form rois_to_csr takes); pairs: (P, 2)
    ROI indices, the candidates; corr: P numbers, one per pair (TracePairCorr.result('corr')).  The pairs with corr >= threshold
    are the edges of a graph on the ROIs, and every connected component becomes ONE ROI: the sorted (flat-index order),
    de-duplicated union of its members' pixels, a (k, 2) int64 array.  SINGLE LINKAGE: it chains -- A-B and B-C accepted merge A
    with C as well, whatever corr(A, C) is or whether (A, C) was a candidate at all.  The output is ordered by smallest flat index
    (then by smallest source ROI, for ROIs that share it); origin[n] is the sorted list of the source ROIs of new_rois[n].  An ROI
    on no accepted edge comes through unchanged (sorted, de-duplicated).  One round per call: a merged ROI has a new trace, and
    merging further is another call on the result.  NaN or a non-number in corr or threshold: ValueError.  Host only."""
    shape = _check_shape(shape)
    W = shape[1]
    threshold = _check_threshold(threshold)
    if not isinstance(pixels, (list, tuple)):
        raise ValueError('pixels must be a list of (k,2) [y,x] arrays, not %s' % type(pixels).__name__)
    flat = _roi_pixels(list(pixels), shape)
    R = len(flat)
    pairs = _check_pairs(pairs, R)
    corr = np.asarray(corr)
    if corr.dtype.kind not in 'fiu':
        raise ValueError('corr must be an array of numbers, one per pair, not %s' % corr.dtype)
    corr = corr.astype(np.float64)
    if corr.shape != (len(pairs),):
        raise ValueError('%d pairs, corr is %r' % (len(pairs), corr.shape))
    if np.isnan(corr).any():
        raise ValueError('corr of pair %d is NaN' % int(np.flatnonzero(np.isnan(corr))[0]))
    root = list(range(R))

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a
    for (i, j), c in zip(pairs.tolist(), corr.tolist()):
        if c >= threshold:
            a, b = find(i), find(j)
            if a != b:
                root[max(a, b)] = min(a, b)          # the smallest member names the component
    members = {}
    for r in range(R):
        members.setdefault(find(r), []).append(r)
    merged = []
    for first, group in members.items():
        p = flat[first] if len(group) == 1 else np.unique(np.concatenate([flat[r] for r in group]))
        merged.append((int(p[0]), first, p, group))
    merged.sort(key=lambda m: m[:2])
    return [_coords(m[2], W) for m in merged], [m[3] for m in merged]


def merge_rois_device(dspath, rois, max_dist=2, threshold=0.8, detrend_frames=None, source='series/raw', device=None, chunk_frames=None,
                      shifts=None, fine_shifts=None, keep=None, bidi=0):
    """-> (new_rois, origin, pairs, corr): merge_rois of `rois` (any form rois_to_csr takes) over `source` of a dataset file.  The
    candidates are roi_neighbours(rois, shape, max_dist); ONE streaming pass through a RoiTraceExtractor gives every ROI's sums, and
    dc_trace_pair_moments / dc_trace_pair_corr run on them where they lie.  With no candidate pair the recording is not read at
    all.  detrend_frames: None, or an integer L in [2, 4096] -- on a recording that bleaches or drifts every trace pair
    correlates; pooling within segments of L frames takes the common trend out (TracePairCorr).  shifts / fine_shifts / bidi: as for
    extract_traces_device.  keep: None, or a (T,) array of booleans (frames.flag_frames): the pairs are correlated over the kept
    columns of the sums only (a torch index, no kernel), and L counts kept frames; all True gives what None gives.
    pairs: int32 (P, 2); corr: float32 (P,)."""
    from ._reader import _read_recording
    from .frames import _check_keep
    from .series import _check_detrend_frames
    from .traces import RoiTraceExtractor
    max_dist = _check_max_dist(max_dist)
    threshold = _check_threshold(threshold)
    if detrend_frames is not None:
        _check_detrend_frames(detrend_frames)
    if keep is not None:
        keep = _check_keep(keep)
    found = []

    def reader_of(shape, T, dtype, **kw):
        """The candidates come from the shape; with none of them there is no reader, and the recording is not read."""
        kept = keep if keep is None else _check_keep(keep, T)
        shape = _check_shape(shape)
        pixels = [_coords(p, shape[1]) for p in _roi_pixels(rois, shape)]
        pairs = roi_neighbours(pixels, shape, max_dist)
        found.extend((shape, pixels, pairs, kept))
        if not len(pairs):
            return None
        # before the GPU is touched or the recording read
        _check_range(T if kept is None else int(kept.sum()), [len(p) for p in pixels], detrend_frames)
        return RoiTraceExtractor(shape, T, dtype, pixels, **kw)
    ext = _read_recording(dspath, source, reader_of, device, chunk_frames, shifts, fine_shifts, bidi)
    shape, pixels, pairs, kept = found
    corr = np.zeros((0,), np.float32)
    if ext is not None:
        sums = ext.sums_device()
        if kept is not None:                     # the kept columns, in order: a fresh contiguous tensor
            import torch
            sums = sums[:, torch.from_numpy(np.flatnonzero(kept)).to(ext.device)]
        corr = TracePairCorr(sums, ext.areas_host(), pairs, detrend_frames=detrend_frames, device=ext.device).result('corr')
    new_rois, origin = merge_rois(pixels, pairs, corr, shape, threshold=threshold)
    return new_rois, origin, pairs, corr
