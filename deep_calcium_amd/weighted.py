"""Weighted ROI traces and overlapping ROIs: footprint-weighted sums on the device, shared pixels excluded or demixed on the host.

RoiFootprints.result('corr') measures how strongly every pixel of an ROI follows the ROI's trace; refine_rois thresholds it and
RoiTraceExtractor then adds the surviving pixels with weight 1, a pixel two ROIs share in full to both.  Here the measurement
becomes a 16-bit integer weight per pixel, the frames are streamed once through dc_roi_wtrace_accumulate (include/dcunet.h,
"Weighted ROI traces"), and the weight sum W_r stands wherever an area stood (finalize, dF/F, trace pairs):

    kind      dtype     what
    sum       int64     sum of w x over the ROI's entries in every frame                  (exact)
    mean      float32   sum / W, the weighted mean                                        (bit-equal to numpy's float64 divide)
    zscore    float32   (trace - mean over time) / population std over time              (exact numerators, <= 1 ulp)
    demix     float64   least-squares coefficients c = G^-1 S per group of overlapping ROIs (numpy's float64 solve: NOT exact)

    rois, weights, kept = footprint_weights(fp.support(), fp.result('corr'), inside=fp.inside(), floor=0.3)
    ext = WeightedTraceExtractor((H, W), T, np.int16, rois, weights)
    for chunk in chunks: ext.feed(chunk)
    S = ext.result('sum')
    C = demix_traces(S, roi_gram(rois, weights, (H, W)))          # shared pixels: each ROI gets its own part

    traces = weighted_traces_device('dataset.hdf5', rois, weights, kind='demix', overlap='demix')

The model behind the demix: pixel p shows x_p(t) = sum_j w_j(p) c_j(t), so the weighted sums are S_i = sum_j G_ij c_j with the Gram
matrix G_ij = sum_p w_i(p) w_j(p), exact integers; c solves G c = S.  The device's part is exact; the solve is a HOST rule in
float64, like split_rois and merge_rois.  Its output is not int64, so dF/F of demixed traces is not offered.

Not built: weights in merge_rois_device, RoiFootprints and RoiPairCorr; a background or neuropil column in the demix; non-negative
or iterated demixing; dF/F of demixed traces; fitting the neuropil weight.

Importing this module needs neither torch nor the GPU; constructing a WeightedTraceExtractor does (there is no CPU fallback).
"""
import numpy as np

from ._reader import _read_recording
from .traces import RoiTraceExtractor, _check_kind, _check_shape, _roi_pixels

MAX_WEIGHT = 65535                    # any uint16 is a legal weight
MAX_WSUM = 2 ** 31 - 1                # DC_WTRACE_MAX_WSUM: W is handed on as an int32 "area"
MAX_VOLUME = 1 << 46                  # DC_WTRACE_MAX_VOLUME: n_frames * W
MAX_COMPONENT = 64                    # ROIs demixed together
UNIT = 256                            # footprint_weights: the weight of a correlation of 1
OVERLAPS = ('keep', 'exclude', 'demix')


def _coords_of(rois):
    if not isinstance(rois, (list, tuple)):
        raise ValueError('rois must be a list of (k,2) [y,x] arrays or region dicts, not %s' % type(rois).__name__)
    if len(rois) == 0:
        raise ValueError('no ROIs')
    return [np.asarray(r['coordinates'] if isinstance(r, dict) else r) for r in rois]


def _weighted_entries(rois, weights, shape, what_zero='refuse'):
    """-> per ROI (flat pixel indices int64, sorted and distinct; weights int64, permuted with them).  Every ValueError names the
    ROI.  weights None: weight 1."""
    H, W = shape
    coords = _coords_of(rois)
    if weights is not None:
        if not isinstance(weights, (list, tuple)) or len(weights) != len(coords):
            raise ValueError('weights must be a list of %d arrays, one per ROI' % len(coords))
    out = []
    for r, c in enumerate(coords):
        if c.size == 0:
            raise ValueError('ROI %d is empty' % r)
        if c.ndim != 2 or c.shape[1] != 2 or c.dtype.kind not in 'iu':
            raise ValueError('ROI %d: coordinates must be a (k,2) integer array of [y,x], not %s %r' % (r, c.dtype, c.shape))
        c = c.astype(np.int64)
        if c.min() < 0 or c[:, 0].max() >= H or c[:, 1].max() >= W:
            raise ValueError('ROI %d has a coordinate outside the %d x %d image' % (r, H, W))
        flat = c[:, 0] * W + c[:, 1]
        order = np.argsort(flat, kind='stable')
        flat = flat[order]
        dup = np.flatnonzero(flat[1:] == flat[:-1])
        if len(dup):
            q = int(flat[dup[0]])
            raise ValueError('ROI %d lists the pixel [%d, %d] more than once' % (r, q // W, q % W))
        if weights is None:
            w = np.ones(len(flat), np.int64)
        else:
            w = np.asarray(weights[r])
            if w.shape != (len(flat),):
                raise ValueError('ROI %d has %d pixels and %s weights' % (r, len(flat), 'x'.join(str(v) for v in w.shape) or 'a scalar of'))
            if w.dtype.kind not in 'iu':
                raise ValueError('ROI %d: weights must be integers in [0, %d], not %s' % (r, MAX_WEIGHT, w.dtype))
            w = w.astype(np.int64) if w.dtype != np.uint64 else np.minimum(w, MAX_WEIGHT + 1).astype(np.int64)
            if w.min() < 0 or w.max() > MAX_WEIGHT:
                raise ValueError('ROI %d: a weight is outside [0, %d]' % (r, MAX_WEIGHT))
            w = w[order]
        out.append((flat, w))
    return out


def _check_wsums(entries, n_frames):
    wsums = []
    for r, (_, w) in enumerate(entries):
        ws = int(w.sum(dtype=np.int64))                     # <= 2^30 entries * 65535: int64 holds it
        if ws == 0:
            raise ValueError('ROI %d: its weights sum to 0' % r)
        if ws > MAX_WSUM:
            raise ValueError('ROI %d: its weights sum to %d, more than 2**31 - 1' % (r, ws))
        if n_frames * ws > MAX_VOLUME:
            raise ValueError('ROI %d: n_frames * weight sum = %d * %d exceeds 2**46' % (r, n_frames, ws))
        wsums.append(ws)
    return np.array(wsums, np.int64)


def _as_coords(flat, W):
    return np.stack([flat // W, flat % W], 1).astype(np.int64)


class WeightedTraceExtractor(RoiTraceExtractor):
    """A RoiTraceExtractor whose accumulate call is dc_roi_wtrace_accumulate: feed() as there, then result()."""
    _stage_tag = 'wtraces_stage'

    def __init__(self, shape, n_frames, dtype, rois, weights, device=None, chunk_frames=None, shifts=None, fine_shifts=None, bidi=0):
        """rois: a list of (k,2) [y,x] arrays or region dicts; weights: a list of (k,) integer arrays in [0, 65535], aligned entry
        by entry with rois as given (they are permuted with the pixels when those are sorted).  The rest as RoiTraceExtractor."""
        # ---- everything that can be wrong with the arguments is a ValueError before the library or the GPU is touched ----
        shape = _check_shape(shape)
        if weights is None:
            raise ValueError('weights must be a list of arrays, one per ROI (RoiTraceExtractor sums with weight 1)')
        try:
            frames_n = int(n_frames)
        except (TypeError, ValueError):
            raise ValueError('n_frames must be an integer, not %r' % (n_frames,))
        entries = _weighted_entries(rois, weights, shape)
        wsums = _check_wsums(entries, max(frames_n, 1))
        row_wgt = np.concatenate([w for _, w in entries]).astype(np.uint16)
        super(WeightedTraceExtractor, self).__init__(shape, n_frames, dtype, [_as_coords(f, shape[1]) for f, _ in entries], device=device,
                                                     chunk_frames=chunk_frames, shifts=shifts, fine_shifts=fine_shifts, bidi=bidi)
        # the base class sorted the same distinct pixels the same way: entry for entry, row_wgt lies beside its row_pix
        assert len(row_wgt) == int(self._row_pix.shape[0])
        self.pixel_counts = self.areas                    # int32[R]: entries per ROI
        self.weight_sums = wsums
        self.areas = wsums.astype(np.int32)               # W_r stands where the area stood (finalize, TraceBaseline, TracePairCorr)
        self._areas = self._torch.from_numpy(self.areas).to(self.device)
        self._row_wgt = self._torch.from_numpy(row_wgt.view(np.int16)).to(self.device)
        self._constructed()

    def _launch(self, fp, tc, t0, st):
        H, W = self.shape
        self.L.dc_roi_wtrace_accumulate(fp, self._unsigned, tc, t0, self._row_off.data_ptr(),
                                        self._row_pix.data_ptr(), self._row_wgt.data_ptr(), self._row_roi.data_ptr(), self._rows,
                                        self.n_rois, self.sums.data_ptr(), self.n_frames, H, W, st)

    def weight_sums_host(self):
        """W_r = the sum of ROI r's weights, int64[R], on the host."""
        return self.weight_sums.copy()

    def areas_host(self):
        """The weight sums as int32[R]: what TraceBaseline and TracePairCorr take as `areas`."""
        return self.areas.copy()


def footprint_weights(coords, corr, inside=None, floor=0.0):
    """-> (rois, weights, kept).  coords / corr / inside: what RoiFootprints.support() / result('corr') / inside() return.  Per entry
    w = floor(256 * max(corr, 0) + 0.5) in float64, NaN -> 0, at most 256.  Entries with corr < floor or w == 0 are dropped, with
    `inside` also every entry outside the ROI's own pixels; ROIs left empty are dropped, and kept indexes the survivors.  rois:
    (k,2) int64 [y,x] in the order given; weights: int64 (k,).  Host numpy only."""
    try:
        floor = float(floor)
    except (TypeError, ValueError):
        raise ValueError('floor must be a number, not %r' % (floor,))
    if floor != floor:
        raise ValueError('floor must be a number, not NaN')
    if len(coords) != len(corr) or (inside is not None and len(inside) != len(coords)):
        raise ValueError('%d supports, %d maps%s' % (len(coords), len(corr), '' if inside is None else ', %d inside masks' % len(inside)))
    rois, weights, kept = [], [], []
    for r, (c, v) in enumerate(zip(coords, corr)):
        c, v = np.asarray(c), np.asarray(v)
        if c.ndim != 2 or c.shape[1] != 2 or c.dtype.kind not in 'iu' or v.shape != (c.shape[0],) or v.dtype.kind not in 'fiu':
            raise ValueError('ROI %d: coordinates must be (k,2) integers and the map (k,) numbers, not %r and %r' % (r, c.shape, v.shape))
        v = v.astype(np.float64)
        nan = v != v
        w = np.floor(UNIT * np.maximum(np.where(nan, 0.0, v), 0.0) + 0.5)
        w = np.minimum(w, UNIT).astype(np.int64)
        keep = (w > 0) & ~(v < floor)
        if inside is not None:
            m = np.asarray(inside[r])
            if m.shape != v.shape or m.dtype != np.bool_:
                raise ValueError('ROI %d: inside must be %d booleans, not %s %r' % (r, len(v), m.dtype, m.shape))
            keep &= m
        if not keep.any():
            continue
        rois.append(c[keep].astype(np.int64))
        weights.append(w[keep])
        kept.append(r)
    return rois, weights, kept


def exclude_overlap(rois, shape, weights=None):
    """-> (rois, weights, kept): every pixel that more than one ROI lists is dropped from all of them (suite2p's
    allow_overlap=False).  ROIs left empty are dropped; kept indexes the survivors.  weights (None: returned as None) follow their
    pixels.  The pixels of every ROI come back in flat-index order.  Host numpy only."""
    shape = _check_shape(shape)
    entries = _weighted_entries(rois, weights, shape)
    count = {}
    for flat, _ in entries:
        for q in flat.tolist():
            count[q] = count.get(q, 0) + 1
    out_r, out_w, kept = [], [], []
    for r, (flat, w) in enumerate(entries):
        own = np.array([count[q] == 1 for q in flat.tolist()], bool)
        if not own.any():
            continue
        out_r.append(_as_coords(flat[own], shape[1]))
        out_w.append(w[own])
        kept.append(r)
    return out_r, (out_w if weights is not None else None), kept


def shared_pixels(rois, shape):
    """The number of pixels of the image that more than one ROI lists."""
    shape = _check_shape(shape)
    flat = np.concatenate([f for f, _ in _weighted_entries(rois, None, shape)])
    _, n = np.unique(flat, return_counts=True)
    return int((n > 1).sum())


def roi_gram(rois, weights, shape):
    """int64 (R,R): G[i,j] = sum over pixels p of w_i(p) w_j(p), exact (w^2 < 2^32 and at most 2^30 pixels: below 2^62).  Built from
    the pixel lists: only pixels that two ROIs share touch an off-diagonal entry.  weights None: weight 1."""
    shape = _check_shape(shape)
    entries = _weighted_entries(rois, weights, shape)
    R = len(entries)
    G = np.zeros((R, R), np.int64)
    for r, (_, w) in enumerate(entries):
        G[r, r] = int((w * w).sum(dtype=np.int64))
    flat = np.concatenate([f for f, _ in entries])
    owner = np.concatenate([np.full(len(f), r, np.int64) for r, (f, _) in enumerate(entries)])
    wgt = np.concatenate([w for _, w in entries])
    order = np.argsort(flat, kind='stable')
    flat, owner, wgt = flat[order], owner[order], wgt[order]
    start = np.flatnonzero(np.concatenate([[True], flat[1:] != flat[:-1]]))
    stop = np.append(start[1:], len(flat))
    for a, b in zip(start.tolist(), stop.tolist()):
        if b - a < 2:
            continue
        for i in range(a, b):
            for j in range(i + 1, b):
                g = int(wgt[i]) * int(wgt[j])
                G[owner[i], owner[j]] += g
                G[owner[j], owner[i]] += g
    return G


def _components(G):
    """The connected components of the graph G[i,j] != 0, each a sorted list, in order of their smallest member."""
    R = len(G)
    parent = list(range(R))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for i, j in zip(*np.nonzero(G)):
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)
    groups = {}
    for r in range(R):
        groups.setdefault(find(r), []).append(r)
    return [groups[k] for k in sorted(groups)]


def bareiss_determinant(rows):
    """The exact determinant of a square matrix of Python ints by fraction-free (Bareiss) elimination: every division is exact."""
    m = [[int(v) for v in row] for row in rows]
    n = len(m)
    sign, prev = 1, 1
    for k in range(n - 1):
        if m[k][k] == 0:
            for i in range(k + 1, n):
                if m[i][k] != 0:
                    m[k], m[i] = m[i], m[k]
                    sign = -sign
                    break
            else:
                return 0
        for i in range(k + 1, n):
            for j in range(k + 1, n):
                m[i][j] = (m[i][j] * m[k][k] - m[i][k] * m[k][j]) // prev
        prev = m[k][k]
    return sign * m[n - 1][n - 1] if n else 1


def demix_traces(sums, gram):
    """float64 (R,T): per connected component c of the graph gram[i,j] != 0 the least-squares coefficients
    np.linalg.solve(G_c, sums_c); an ROI that shares no pixel gives sums / G_ii.  sums: (R,T) integers (WeightedTraceExtractor's
    result('sum')), gram: roi_gram's.  A component is refused, its ROIs named, when its exact integer determinant is 0 (two
    identical footprints) or it has more than 64 ROIs.  A HOST rule in float64 on exact integers: not exact, and not int64, so
    there is no dF/F of demixed traces."""
    S, G = np.asarray(sums), np.asarray(gram)
    if S.ndim != 2 or S.dtype.kind not in 'iu':
        raise ValueError('sums must be an (R,T) integer matrix, not %s %r' % (S.dtype, S.shape))
    R = S.shape[0]
    if G.shape != (R, R) or G.dtype.kind not in 'iu' or not np.array_equal(G, G.T):
        raise ValueError('gram must be a symmetric (%d,%d) integer matrix, not %s %r' % (R, R, G.dtype, G.shape))
    out = np.empty(S.shape, np.float64)
    for comp in _components(G):
        if len(comp) > MAX_COMPONENT:
            raise ValueError('the ROIs %s overlap in one group of %d: more than %d are not demixed together' % (comp, len(comp), MAX_COMPONENT))
        Gc = G[np.ix_(comp, comp)]
        if bareiss_determinant(Gc.tolist()) == 0:
            raise ValueError('the ROIs %s have linearly dependent footprints (determinant 0): they cannot be demixed' % (comp,))
        if len(comp) == 1:
            out[comp[0]] = S[comp[0]].astype(np.float64) / np.float64(Gc[0, 0])
        else:
            out[comp] = np.linalg.solve(Gc.astype(np.float64), S[comp].astype(np.float64))
    return out


def zscore64(x):
    """(x - mean over time) / population std over time in float64 numpy; a row that is constant in time gives 0."""
    x = np.asarray(x, np.float64)
    d = x - x.mean(axis=1, keepdims=True)
    sd = np.sqrt((d * d).mean(axis=1, keepdims=True))
    return np.where(sd > 0, d / np.where(sd > 0, sd, 1.0), 0.0)


def _check_overlap(overlap, kind):
    if overlap not in OVERLAPS:
        raise ValueError('overlap %r is not one of %s' % (overlap, ', '.join(OVERLAPS)))
    if overlap == 'demix':
        if kind not in ('demix', 'zscore'):
            raise ValueError("with overlap='demix' the kind is 'demix' or 'zscore', not %r" % (kind,))
    else:
        _check_kind(kind)


def _prepare(rois, weights, shape, overlap):
    """-> (rois, weights) as lists for WeightedTraceExtractor.  weights None: weight 1 and every form of rois rois_to_csr takes."""
    if weights is None:
        rois = [_as_coords(p.astype(np.int64), shape[1]) for p in _roi_pixels(rois, shape)]
        weights = [np.ones(len(c), np.int64) for c in rois]
    if overlap == 'exclude':
        n = len(rois)
        rois, weights, kept = exclude_overlap(rois, shape, weights)
        if len(kept) != n:
            lost = sorted(set(range(n)) - set(kept))
            raise ValueError('ROI %d has no pixel of its own left once shared pixels are excluded (ROIs lost: %s): call exclude_overlap and pass what '
                             'it keeps' % (lost[0], lost))
    return list(rois), list(weights)


def weighted_traces_device(dspath, rois, weights=None, kind='mean', overlap='keep', source='series/raw', device=None, chunk_frames=None,
                           shifts=None, fine_shifts=None, bidi=0):
    """The (R,T) weighted traces of `rois` over `source` of a dataset file, in one pass.  weights: one integer array per ROI, or None
    for weight 1 (then rois may take every form rois_to_csr takes).  overlap: 'keep' (a shared pixel counts for every ROI that lists
    it), 'exclude' (shared pixels are dropped first; an ROI left without a pixel is a ValueError), 'demix' (demix_traces of the
    sums; kind is then 'demix', the float64 coefficients, or 'zscore', their population z-score in float64 numpy).  shifts /
    fine_shifts / bidi: as for extract_traces_device."""
    _check_overlap(overlap, kind)
    gram = []

    def reader_of(shape, n_frames, dtype, **kw):
        shape = _check_shape(shape)
        own, wgt = _prepare(rois, weights, shape, overlap)
        if overlap == 'demix':
            gram.append(roi_gram(own, wgt, shape))
            demix_traces(np.zeros((len(gram[0]), 1), np.int64), gram[0])    # a group that cannot be demixed: before the pass, not after it
        return WeightedTraceExtractor(shape, n_frames, dtype, own, wgt, **kw)
    ext = _read_recording(dspath, source, reader_of, device, chunk_frames, shifts, fine_shifts, bidi)
    if overlap != 'demix':
        return ext.result(kind)
    out = demix_traces(ext.result('sum'), gram[0])
    return zscore64(out) if kind == 'zscore' else out
