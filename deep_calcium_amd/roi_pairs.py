"""Splitting merged ROIs: the correlation over time of every pixel of an ROI with every other pixel of it, and a two-way split.

An ROI of the chain is an 8-connected region of a mask predicted from ONE summary image (traces._roi_pixels), so two cells that
touch are one ROI with one trace, and z-score, dF/F and the spikes model inherit the mix.  The footprint map (footprints.py)
cannot separate them: both halves correlate with the summed trace.  The correlation of the pixels with EACH OTHER can.  The
reference has no counterpart; the definitions in include/dcunet.h ("ROI pixel-pair correlation") are the specification.  The
frames are streamed once through dc_roi_trace_accumulate and dc_roi_pair_accumulate, chunk by chunk on the same stream, so one
pass gives the matrices AND the traces:

    kind        dtype     what
    moments     int       a_i = sum x_i, g_ij = sum x_i x_j of every ROI's own pixels                  (exact)
    corr        float32   corr(x_i, x_j), a (k, k) matrix per ROI                                      (exact numerators, <= 1 ulp)

    pc = RoiPairCorr((H, W), T, np.int16, rois)
    for chunk in chunks: pc.feed(chunk)           # numpy / memmap chunks, or an int16 CUDA tensor that is already resident
    C = pc.result('corr')                         # list of R float32 (k, k), bit-symmetric, aligned with pc.pixels()
    new_rois, origin, gaps = split_rois(pc.pixels(), C, (H, W), min_gap=0.1, min_area=8)

    new_rois, origin, gaps = split_rois_device('dataset.hdf5', mask)          # one call, one pass

A pixel that is constant in time (a single frame included) has a row, a column and a diagonal of exactly 0 here; numpy divides
0 by 0 there.  An ROI may have at most MAX_AREA pixels, and all ROIs together MAX_STATE matrix entries.

The split rule (split_rois; host numpy in float64, deterministic).  For each ROI, C is its matrix, diagonal included:
 1. i0 = argmax_i sum_j C[i, j]; j0 = argmax_j ||C[j, :] - C[i0, :]||^2; the first index wins ties.  The centres are rows i0, j0.
 2. Lloyd iterations on the rows with squared Euclidean distance: a row goes to the nearer centre, a tie to centre 0; a centre
    becomes the mean of its rows.  Stop when the labels repeat or after `iterations` assignments.  An empty cluster: the ROI is
    kept unsplit.
 3. Each part is the largest 8-connected component of its cluster (nf_metrics.mask_to_regions; a tie goes to the component that
    holds the smallest flat index); the other pixels of the ROI are dropped from both parts, as refine_rois drops them.
 4. within_* = the mean of C over the part's off-diagonal pairs, between = the mean over the pairs across the two parts,
    gap = min(within_a, within_b) - between.  The split is accepted only if both parts have at least min_area pixels and
    gap >= min_gap.  The min is essential: a single cell with a bright centre and a dim rim clusters into centre and rim, and its
    dim cluster has a low `within`; with an average in place of the minimum such a cell approaches the threshold.
 5. The parts of a split ROI are consecutive entries of the output, ordered by their smallest flat index; an unsplit ROI comes
    through unchanged.  One two-way split per ROI per call: splitting further is another call, and another pass, on the result.

The rule's reach, on a 6 x 12 region of two 6 x 6 cells, T = 256, independent Poisson spikes (rate 0.03, decay 8 frames) over a
baseline of 400 with a shared neuropil trace at 0.3 of the amplitude, 40 seeds each: at amplitude 60 and pixel noise sigma 30 the
two cells are split in 38 scenes with no pixel misassigned or dropped (the other two hold a cell that fires once, or four times),
and a single cell (uniform or with a Gaussian profile) and a static region never are; at amplitude 40 / sigma 40 the two cells are
split in 12 of 40 scenes, at 30 / 60 in none.

A recording that bleaches or drifts: a decay common to all pixels pushes every correlation towards 1 and hides the two groups (on
the scene above at T = 1024, a decay to half the brightness takes the rule from 40 of 40 scenes to 0).  detrend_frames=L correlates
within segments of L frames and pools them (series.detrend_plan, dc_roi_pair_fold_segment, dc_roi_pair_corr_pooled): all 40 come
back at L = 128 with no pixel wrong.  Short segments also remove real slow covariance (at amplitude 40 / sigma 40 without decay: 21
scenes with None, 15 at L = 128, 8 at L = 64): use the longest L that removes the trend.

Importing this module needs neither torch nor the GPU; constructing a RoiPairCorr does (there is no CPU fallback).
"""
import numpy as np

from ._reader import _check_n_frames, _read_recording
from .dff import _as_int
from .footprints import MAX_FRAMES, _largest_component
from .traces import MAX_VOLUME, _LeadingExtractor, _check_shape, _roi_pixels

KINDS = ('moments', 'corr')
TILE = 64                             # DC_ROI_PAIR_TILE: the edge, in pairs, of one workgroup's tile of an ROI's square
BATCH = 32                            # DC_ROI_PAIR_BATCH: the frames the kernel stages at a time
MAX_AREA = 1024                       # DC_ROI_PAIR_MAX_AREA: pixels per ROI
MAX_STATE = 1 << 27                   # DC_ROI_PAIR_MAX_STATE: sum of k^2 over the ROIs (1 GiB of int64)


def _check_kind(kind):
    if kind not in KINDS:
        raise ValueError('pair kind %r is not one of %s' % (kind, ', '.join(KINDS)))


def pair_layout(areas):
    """areas: the pixel count k of every ROI -> (roi_off int32[R+1], goff int64[R], tiles int32[ntiles, 3], G): ROI r's pixels are
    entries roi_off[r]..roi_off[r+1] of the pixel list, its k x k square lies at goff[r] of a state of G = sum k^2 words, and
    tiles lists (r, ti, tj) for every ti <= tj < ceil(k / TILE), ROI by ROI, row by row: what dc_roi_pair_accumulate takes.
    ValueError, naming the ROI, where k > MAX_AREA or the state passes MAX_STATE.  Host only."""
    areas = [int(k) for k in areas]
    roi_off, goff, tiles, G = [0], [], [], 0
    for r, k in enumerate(areas):
        if k < 1:
            raise ValueError('ROI %d is empty' % r)
        if k > MAX_AREA:
            raise ValueError('ROI %d has %d pixels: the pair correlation is limited to %d per ROI' % (r, k, MAX_AREA))
        goff.append(G)
        G += k * k
        if G > MAX_STATE:
            raise ValueError('ROI %d brings the pair state to %d entries: limited to 2**27 = %d' % (r, G, MAX_STATE))
        roi_off.append(roi_off[-1] + k)
        nt = (k + TILE - 1) // TILE
        tiles += [(r, ti, tj) for ti in range(nt) for tj in range(ti, nt)]
    return (np.array(roi_off, np.int32), np.array(goff, np.int64).reshape(-1), np.array(tiles, np.int32).reshape(-1, 3), G)


class RoiPairCorr(object):
    """Owns the device state of one recording's pixel-pair moments and, through a RoiTraceExtractor of its own, of its traces;
    feed() the frames in order, in chunks of any size, then result()."""

    def __init__(self, shape, n_frames, dtype, rois, device=None, chunk_frames=None, shifts=None, fine_shifts=None, detrend_frames=None,
                 bidi=0):
        """rois: every form rois_to_csr takes; each ROI at most MAX_AREA pixels, all together at most MAX_STATE matrix entries
        (ValueError naming the ROI).  Everything else: as for RoiTraceExtractor (bidi, then shifts / fine_shifts move or interpolate each
        chunk before BOTH kernels read it).
        detrend_frames: None, or an integer L in [2, 4096]: the matrices are formed from centred moments pooled over the segments
        of series.detrend_plan(n_frames, L) (dc_roi_pair_fold_segment at every segment's end, dc_roi_pair_corr_pooled): a trend
        that is constant within a segment is removed.  L > n_frames / 2 is one segment: the bits of None.  The traces of the same
        pass are not detrended."""
        # ---- everything that can be wrong with the arguments is a ValueError before the library or the GPU is touched ----
        shape = _check_shape(shape)
        n_frames = _check_n_frames(n_frames, shape, max_volume=MAX_VOLUME)
        if n_frames > MAX_FRAMES:
            raise ValueError('n_frames must be <= 2**31 - 1, not %d' % n_frames)
        self._seg = None
        if detrend_frames is not None:
            from .series import _Segments, _check_detrend_frames
            self._seg = _Segments(n_frames, _check_detrend_frames(detrend_frames, n_frames, shape))
        pixels = _roi_pixels(rois, shape)
        roi_off, goff, tiles, G = pair_layout([len(p) for p in pixels])
        self._pixels = [np.stack([p.astype(np.int64) // shape[1], p.astype(np.int64) % shape[1]], 1) for p in pixels]
        self._roi_off_host, self._goff_host = roi_off.astype(np.int64), goff
        self.n_pixels, self.n_state, self.n_tiles = int(roi_off[-1]), G, len(tiles)
        # slots of its own: an extractor alive at the same time keeps its own
        self._ext = ext = _LeadingExtractor('roi_pairs_stage', self._accumulate, shape, n_frames, dtype, self._pixels, device=device,
                                            chunk_frames=chunk_frames, shifts=shifts, fine_shifts=fine_shifts, bidi=bidi)
        self.shape, self.n_frames, self.dtype, self.n_rois = shape, n_frames, ext.dtype, ext.n_rois
        self.chunk_frames, self.device, self.L = ext.chunk_frames, ext.device, ext.L
        torch = self._torch = ext._torch
        dev = self.device
        self._roi_off = torch.from_numpy(roi_off).to(dev)
        self._roi_pix = torch.from_numpy(np.concatenate(pixels).astype(np.int32)).to(dev)
        self._goff = torch.from_numpy(goff).to(dev)
        self._tiles = torch.from_numpy(np.ascontiguousarray(tiles)).to(dev)
        self._a = torch.zeros((self.n_pixels,), dtype=torch.int64, device=dev)           # the kernel adds
        self._g = torch.zeros((G,), dtype=torch.int64, device=dev)
        self._pooled = torch.zeros((G, 2), dtype=torch.int64, device=dev) if self._seg is not None else None      # 16-byte {lo, hi} words
        self._corr = None
        ext._constructed()               # again: the fills above belong to what its feed() waits for

    @property
    def fed(self):
        return self._ext.fed

    def _accumulate(self, fp, tc, t0, st):
        H, W = self.shape
        if self._seg is not None:        # cut at the segment boundaries; a segment that ends is folded, which leaves a and g zero
            for k, m, _, ends in self._seg.cut(t0, tc):
                self._accumulate_frames(fp + k * H * W * 2, m, st)
                if ends is not None:
                    self.L.dc_roi_pair_fold_segment(self._a.data_ptr(), self._g.data_ptr(), self._roi_off.data_ptr(), self._goff.data_ptr(),
                                                    self._tiles.data_ptr(), self.n_tiles, self.n_rois, self.n_pixels, self.n_state,
                                                    ends[1], ends[2], self._pooled.data_ptr(), st)
            return
        self._accumulate_frames(fp, tc, st)

    def _accumulate_frames(self, fp, tc, st):
        H, W = self.shape
        self.L.dc_roi_pair_accumulate(fp, int(self.dtype == np.dtype(np.uint16)), tc, self._roi_off.data_ptr(), self._roi_pix.data_ptr(),
                                      self._goff.data_ptr(), self._tiles.data_ptr(), self.n_tiles, self.n_rois, self._a.data_ptr(),
                                      self._g.data_ptr(), self.n_pixels, self.n_state, H, W, st)

    def feed(self, frames):
        """The next frames of the recording: what RoiTraceExtractor.feed takes.  Per chunk dc_roi_trace_accumulate and then
        dc_roi_pair_accumulate run on the same stream on the same frames."""
        self._ext.feed(frames)
        return self

    def pixels(self):
        """Per ROI the (k,2) int64 [y,x] of its pixels, in flat-index order: the rows and columns of its matrix."""
        return [p.copy() for p in self._pixels]

    def traces(self, kind='mean'):
        """RoiTraceExtractor.result(kind) of the same pass.  Fed the output of a series.TemporalBinner, these are the traces of the
        BINNED recording (n_frames // bin_frames samples of rounded means): a trace of every frame is another, unbinned pass."""
        return self._ext.result(kind)

    def _squares(self, flat):
        out = []
        for r in range(self.n_rois):
            k = int(self._roi_off_host[r + 1] - self._roi_off_host[r])
            out.append(flat[self._goff_host[r]:self._goff_host[r] + k * k].reshape(k, k))
        return out

    def _corr_flat(self):
        if self._corr is None:
            torch = self._torch
            with torch.cuda.device(self.device):
                st = torch.cuda.current_stream(self.device).cuda_stream
                corr = torch.empty((self.n_state,), dtype=torch.float32, device=self.device)
                if self._seg is not None:
                    self.L.dc_roi_pair_corr_pooled(self._pooled.data_ptr(), self._roi_off.data_ptr(), self._goff.data_ptr(), self.n_rois,
                                                   self.n_pixels, self.n_state, corr.data_ptr(), st)
                else:
                    self.L.dc_roi_pair_corr(self._a.data_ptr(), self._g.data_ptr(), self._roi_off.data_ptr(), self._goff.data_ptr(), self.n_rois,
                                            self.n_pixels, self.n_state, self.n_frames, corr.data_ptr(), st)
            self._corr = corr.cpu().numpy()
        return self._corr

    def result(self, kind='corr'):
        """'corr': a list of R float32 (k, k) matrices aligned with pixels(); 'moments': per ROI a dict of object arrays of exact
        Python ints, a (k,) and g (k, k), g symmetric (the device keeps i <= j; the other half is mirrored here) -- with
        detrend_frames: dict(N (k, k) symmetric, the pooled numerators; M)."""
        _check_kind(kind)
        if self.fed != self.n_frames:
            raise ValueError('result() after %d of %d frames' % (self.fed, self.n_frames))
        if kind == 'corr':
            return [c.copy() for c in self._squares(self._corr_flat())]
        if self._seg is not None:        # the pooled numerators N(x_i, x_j), exact, with M: integers before any float
            from .series import _pooled_ints
            out = []
            for n in self._squares(_pooled_ints(self._pooled.cpu().numpy())):
                n = np.triu(n)
                out.append(dict(N=n + np.triu(n, 1).T, M=self._seg.M))
            return out
        a = self._a.cpu().numpy().astype(object)
        out = []
        for r, g in enumerate(self._squares(self._g.cpu().numpy())):
            g = np.triu(g)
            g = (g + np.triu(g, 1).T).astype(object)
            out.append(dict(a=a[self._roi_off_host[r]:self._roi_off_host[r + 1]], g=g))
        return out


def _check_split_args(min_gap, min_area, iterations):
    min_area = _as_int(min_area, 'min_area')
    if min_area < 1:
        raise ValueError('min_area must be >= 1, not %d' % min_area)
    iterations = _as_int(iterations, 'iterations')
    if iterations < 1:
        raise ValueError('iterations must be >= 1, not %d' % iterations)
    try:
        min_gap = float(min_gap)
    except (TypeError, ValueError):
        raise ValueError('min_gap must be a number, not %r' % (min_gap,))
    if min_gap != min_gap:
        raise ValueError('min_gap must be a number, not NaN')
    return min_gap, min_area, iterations


def _split_one(c, C, W, min_gap, min_area, iterations):
    """-> (parts or None, gap).  c: (k,2) in flat-index order, C: float64 (k,k)."""
    i0 = int(np.argmax(C.sum(1)))
    j0 = int(np.argmax(((C - C[i0]) ** 2).sum(1)))
    c0, c1 = C[i0].copy(), C[j0].copy()
    labels = None
    for _ in range(iterations):
        new = ((C - c1) ** 2).sum(1) < ((C - c0) ** 2).sum(1)          # a tie goes to centre 0
        if labels is not None and np.array_equal(new, labels):
            break
        labels = new
        if new.all() or not new.any():
            return None, np.nan
        c0, c1 = C[~new].mean(0), C[new].mean(0)
    flat = c[:, 0] * W + c[:, 1]
    index = dict((int(f), n) for n, f in enumerate(flat))
    parts, members = [], []
    for side in (False, True):
        p = _largest_component(c[labels == side])
        parts.append(p)
        members.append(np.array([index[int(f)] for f in p[:, 0] * W + p[:, 1]]))
    if min(len(m) for m in members) < 2:
        return None, np.nan                          # a part of one pixel has no pairs
    within = []
    for m in members:
        sub = C[np.ix_(m, m)]
        within.append((sub.sum() - np.trace(sub)) / (len(m) * (len(m) - 1)))
    between = C[np.ix_(members[0], members[1])].mean()
    gap = float(min(within) - between)
    if min(len(p) for p in parts) < min_area or not gap >= min_gap:
        return None, gap
    parts.sort(key=lambda p: int(p[0, 0]) * W + int(p[0, 1]))
    return parts, gap


def split_rois(pixels, corr, shape, min_gap=0.1, min_area=8, iterations=16):
    """-> (new_rois, origin, gaps): the two-way split of every ROI whose pixel-pair correlation shows two groups (the rule: the
    module's docstring).  pixels / corr: what RoiPairCorr.pixels() / result('corr') return -- per ROI a (k,2) [y,x] array in
    flat-index order and its (k,k) matrix; a matrix of None, or an ROI of fewer than 2 * min_area pixels, is passed through
    without clustering.  new_rois: (k,2) int64 arrays, the two parts of a split ROI consecutive and ordered by smallest flat
    index, an unsplit ROI unchanged; origin[n]: the ROI new_rois[n] came from; gaps: float64 (R,), the gap found, NaN where no
    clustering was attempted or it left a part without pairs.  Host numpy only."""
    H, W = _check_shape(shape)
    min_gap, min_area, iterations = _check_split_args(min_gap, min_area, iterations)
    if len(pixels) != len(corr):
        raise ValueError('%d ROIs, %d matrices' % (len(pixels), len(corr)))
    new_rois, origin, gaps = [], [], np.full(len(pixels), np.nan, np.float64)
    for r, (c, C) in enumerate(zip(pixels, corr)):
        c = np.asarray(c)
        if c.ndim != 2 or c.shape[1] != 2 or c.dtype.kind not in 'iu' or len(c) == 0:
            raise ValueError('ROI %d: coordinates must be a non-empty (k,2) integer array, not %s %r' % (r, c.dtype, c.shape))
        c = c.astype(np.int64)
        if c.min() < 0 or c[:, 0].max() >= H or c[:, 1].max() >= W:
            raise ValueError('ROI %d has a coordinate outside the %d x %d image' % (r, H, W))
        if (np.diff(c[:, 0] * W + c[:, 1]) <= 0).any():
            raise ValueError('ROI %d: the pixels are not in flat-index order' % r)
        parts = None
        if C is not None:
            C = np.asarray(C)
            if C.shape != (len(c), len(c)) or C.dtype.kind != 'f':
                raise ValueError('ROI %d: the matrix must be float (%d, %d), not %s %r' % (r, len(c), len(c), C.dtype, C.shape))
            if len(c) >= 2 * min_area:
                parts, gaps[r] = _split_one(c, C.astype(np.float64), W, min_gap, min_area, iterations)
        for p in ([c] if parts is None else parts):
            new_rois.append(p)
            origin.append(r)
    return new_rois, origin, gaps


def roi_pair_corr_device(dspath, rois, source='series/raw', device=None, chunk_frames=None, shifts=None, fine_shifts=None,
                         bin_frames=None, detrend_frames=None, keep=None, bidi=0):
    """-> (corr, pixels) of `rois` (any form rois_to_csr takes) over `source` of a dataset file, streamed chunk by chunk: the
    recording is read once.  shifts / fine_shifts / bidi: as for extract_traces_device.  bin_frames: None, or an integer b in
    [1, 64]: the matrices are those of the T // b rounded means of b consecutive corrected frames (series.TemporalBinner; the
    trailing T % b frames are dropped, 1 gives what None gives).  detrend_frames: None, or an integer L in [2, 4096]: the
    correlations are pooled over segments of L frames (RoiPairCorr); binning comes first and L counts binned frames.  keep: None, or
    a (T,) array of booleans (frames.flag_frames): the frames marked False are left out after bidi and the shifts and before binning
    and detrending, whose b and L then count kept frames; all True gives what None gives."""
    from .series import _check_detrend_frames
    if detrend_frames is not None:
        _check_detrend_frames(detrend_frames)

    def reader_of(shape, n_frames, dtype, **kw):
        return RoiPairCorr(shape, n_frames, dtype, rois, detrend_frames=detrend_frames, **kw)
    pc = _read_recording(dspath, source, reader_of, device, chunk_frames, shifts, fine_shifts, bidi, bin_frames, keep)
    return pc.result('corr'), pc.pixels()


def split_rois_device(dspath, rois, min_gap=0.1, min_area=8, iterations=16, source='series/raw', device=None, chunk_frames=None,
                      shifts=None, fine_shifts=None, bin_frames=None, detrend_frames=None, keep=None, bidi=0):
    """-> (new_rois, origin, gaps) of split_rois for `rois` over `source` of a dataset file, in one pass over the recording.  ROIs
    of more than MAX_AREA or fewer than 2 * min_area pixels are not sent to the device and come back unchanged (gap NaN); when
    no ROI is left the recording is not read at all.  shifts / fine_shifts / bidi: as for extract_traces_device.  bin_frames: as
    for roi_pair_corr_device -- the pixel noise of a mean of b frames is lower by sqrt(b), which is what lets the rule part cells
    it cannot part frame by frame; keep T // b well above 100, chance correlations split static regions below that.  detrend_frames:
    as for roi_pair_corr_device -- a decay common to all pixels pushes every whole-recording correlation towards 1 and hides the
    two groups; pooling over segments of L frames gives them back.  Short segments also remove real slow covariance: results at
    different L are not comparable with each other or with None.  keep: as for roi_pair_corr_device -- three flash frames in a
    thousand push every pixel pair towards 1 as bleaching does; leaving them out gives the two groups back."""
    from .series import _check_bin_frames, _check_detrend_frames
    if detrend_frames is not None:
        _check_detrend_frames(detrend_frames)
    min_gap, min_area, iterations = _check_split_args(min_gap, min_area, iterations)
    if bin_frames is not None:
        _check_bin_frames(bin_frames)
    if keep is not None:
        from .frames import _check_keep
        keep = _check_keep(keep)
    shape = []                               # the frame shape alone: a reader of None reads nothing
    _read_recording(dspath, source, lambda hw, n_frames, dtype, **kw: shape.extend(hw), shifts=shifts, fine_shifts=fine_shifts, bidi=bidi)
    shape = _check_shape(shape)
    flat = _roi_pixels(rois, shape)
    pixels = [np.stack([p.astype(np.int64) // shape[1], p.astype(np.int64) % shape[1]], 1) for p in flat]
    sent = [r for r, p in enumerate(pixels) if 2 * min_area <= len(p) <= MAX_AREA]
    corr = [None] * len(pixels)
    if sent:
        got, _ = roi_pair_corr_device(dspath, [pixels[r] for r in sent], source=source, device=device, chunk_frames=chunk_frames,
                                      shifts=shifts, fine_shifts=fine_shifts, bidi=bidi, bin_frames=bin_frames, detrend_frames=detrend_frames,
                                      keep=keep)
        for r, c in zip(sent, got):
            corr[r] = c
    return split_rois(pixels, corr, shape, min_gap=min_gap, min_area=min_area, iterations=iterations)
