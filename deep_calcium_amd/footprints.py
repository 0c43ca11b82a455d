"""ROI footprint maps on the device: the correlation over time of every pixel of an ROI's support with the ROI's own trace.

The ROIs of the chain are the regions of a mask predicted from ONE summary image (traces._roi_pixels): a static bright structure
becomes a "neuron", two touching cells one ROI, a mask a pixel too fat dilutes its trace with neuropil.  This module checks every
ROI against the recording it came from.  The reference has no counterpart; the definitions in include/dcunet.h ("ROI footprint
maps") are the specification.  The frames are streamed once through dc_roi_trace_accumulate and dc_roi_pixel_accumulate, chunk by
chunk on the same stream, so one pass gives the maps AND the traces:

    kind        dtype     what
    moments     int       a = sum x, b = sum x^2, c = sum x S of every support entry                  (exact)
    corr        float32   corr(x, S) for a halo entry, corr(x, S - x) for an entry inside the ROI     (exact numerators, <= 1 ulp)
    coherence   float64   per ROI: the mean of corr over its inside entries                            (numpy's float64 mean)

    fp = RoiFootprints((H, W), T, np.int16, rois, halo=2)
    for chunk in chunks: fp.feed(chunk)           # numpy / memmap chunks, or an int16 CUDA tensor that is already resident
    corr = fp.result('corr')                      # list of R float32 arrays, aligned with fp.support() and fp.inside()
    traces = fp.traces('zscore')                  # the same pass's traces
    new_rois, kept = refine_rois(fp.support(), corr, (H, W), threshold=0.3)

    corr, coords, inside = roi_footprints_device('dataset.hdf5', mask, halo=2)

A pixel or a trace that is constant in time (a single frame included) and the pixel of a one-pixel ROI have a correlation of
exactly 0 here; numpy divides 0 by 0 there.  The map cannot split one ROI into two (both halves correlate with the summed trace,
and refine_rois keeps the larger): roi_pairs.py does, from the correlation of the ROI's pixels with each other.

detrend_frames=L: pixel and trace are correlated within segments of L frames and the segments pooled (series.detrend_plan,
dc_roi_pixel_fold_segment, dc_roi_pixel_corr_pooled), so that bleaching and drift common to all pixels do not push every entry of
the map towards 1.  Piecewise-constant detrending: a trend inside a segment stays.

Importing this module needs neither torch nor the GPU; constructing a RoiFootprints does (there is no CPU fallback).
"""
import numpy as np

from ._reader import _check_n_frames, _read_recording
from .dff import _as_int, _dilate
from .traces import MAX_VOLUME, _LeadingExtractor, _check_shape, _roi_pixels, rois_to_csr

KINDS = ('moments', 'corr', 'coherence')
MAX_HALO = 16
MAX_FRAMES = 2147483647               # DC_ROI_PIXEL_MAX_FRAMES: b = sum x^2 stays below 2^63


def _check_kind(kind):
    if kind not in KINDS:
        raise ValueError('footprint kind %r is not one of %s' % (kind, ', '.join(KINDS)))


def _check_halo(halo):
    halo = _as_int(halo, 'halo')
    if not 0 <= halo <= MAX_HALO:
        raise ValueError('halo must be an integer in [0, %d], not %d' % (MAX_HALO, halo))
    return halo


def _support(pixels, shape, halo):
    """pixels: traces._roi_pixels -> per ROI the sorted flat indices of the support and the bool `inside` beside them."""
    H, W = shape
    flat, inside = [], []
    for p in pixels:
        p = p.astype(np.int64)
        y, x = p // W, p % W
        y0, y1 = max(0, int(y.min()) - halo), min(H, int(y.max()) + halo + 1)      # the support cannot leave this box
        x0, x1 = max(0, int(x.min()) - halo), min(W, int(x.max()) + halo + 1)
        own = np.zeros((y1 - y0, x1 - x0), bool)
        own[y - y0, x - x0] = True
        c = np.argwhere(_dilate(own, halo))          # raster order: sorted by flat index
        flat.append((c[:, 0] + y0) * W + (c[:, 1] + x0))
        inside.append(own[c[:, 0], c[:, 1]])
    return flat, inside


def roi_support(rois, shape, halo=2):
    """-> (coords, inside): per ROI a (k,2) int64 array of [y,x] and a bool (k,).  The support of an ROI is its own pixels (inside)
    plus every pixel of the image within Chebyshev distance `halo` of one of them (halo), sorted by flat index y * W + x and
    de-duplicated.  Pixels of other ROIs are not excluded.  `rois`: every form rois_to_csr takes.  Host numpy only."""
    shape = _check_shape(shape)
    halo = _check_halo(halo)
    flat, inside = _support(_roi_pixels(rois, shape), shape, halo)
    return [np.stack([f // shape[1], f % shape[1]], 1).astype(np.int64) for f in flat], inside


def _largest_component(c):
    """c: (n,2) integer [y,x], n >= 1 -> its largest 8-connected component as (m,2) int64 in flat-index order (labelled by
    nf_metrics.mask_to_regions; ties: the component that holds the smallest flat index)."""
    from .nf_metrics import mask_to_regions
    y0, x0 = c.min(0)
    m = np.zeros((int(c[:, 0].max() - y0) + 1, int(c[:, 1].max() - x0) + 1), bool)
    m[c[:, 0] - y0, c[:, 1] - x0] = True
    regions = mask_to_regions(m)                     # raster label order: the first of the largest holds the smallest flat index
    best = regions[int(np.argmax([len(g) for g in regions]))]
    return (best + np.array([y0, x0])).astype(np.int64)


def refine_rois(coords, corr, shape, threshold=0.3, min_area=1):
    """-> (new_rois, kept).  Per ROI: the entries with corr >= threshold, of those the largest 8-connected component (ties: the one
    that holds the smallest flat index; labelled by nf_metrics.mask_to_regions), dropped if fewer than min_area pixels remain.
    new_rois: the survivors as (k,2) int64 [y,x] arrays in flat-index order; kept: the indices of the ROIs they came from.
    coords / corr: what RoiFootprints.support() / result('corr') return.  Host numpy only."""
    H, W = _check_shape(shape)
    min_area = _as_int(min_area, 'min_area')
    if min_area < 1:
        raise ValueError('min_area must be >= 1, not %d' % min_area)
    try:
        threshold = float(threshold)
    except (TypeError, ValueError):
        raise ValueError('threshold must be a number, not %r' % (threshold,))
    if threshold != threshold:
        raise ValueError('threshold must be a number, not NaN')
    if len(coords) != len(corr):
        raise ValueError('%d supports, %d maps' % (len(coords), len(corr)))
    new_rois, kept = [], []
    for r, (c, v) in enumerate(zip(coords, corr)):
        c, v = np.asarray(c), np.asarray(v)
        if c.ndim != 2 or c.shape[1] != 2 or c.dtype.kind not in 'iu' or v.shape != (c.shape[0],):
            raise ValueError('ROI %d: coordinates must be (k,2) integers and the map (k,), not %r and %r' % (r, c.shape, v.shape))
        if c.size and (c.min() < 0 or c[:, 0].max() >= H or c[:, 1].max() >= W):
            raise ValueError('ROI %d has a coordinate outside the %d x %d image' % (r, H, W))
        c = c[v.astype(np.float64) >= threshold]     # compared as doubles, whatever the map's dtype
        if len(c) == 0:
            continue
        best = _largest_component(c)
        if len(best) < min_area:
            continue
        new_rois.append(best)
        kept.append(r)
    return new_rois, kept


class RoiFootprints(object):
    """Owns the device state of one recording's footprint maps and, through a RoiTraceExtractor of its own, of its traces; feed()
    the frames in order, in chunks of any size, then result()."""

    def __init__(self, shape, n_frames, dtype, rois, halo=2, device=None, chunk_frames=None, shifts=None, fine_shifts=None, detrend_frames=None,
                 bidi=0):
        """halo: the Chebyshev radius, in [0, 16], by which every ROI's support reaches beyond its own pixels.  Everything else: as
        for RoiTraceExtractor (bidi, then shifts / fine_shifts move or interpolate each chunk before BOTH kernels read it).
        detrend_frames: None, or an integer L in [2, 4096]: the maps are formed from centred moments pooled over the segments of
        series.detrend_plan(n_frames, L) (dc_roi_trace_moments over the segment's columns and dc_roi_pixel_fold_segment at every
        segment's end, dc_roi_pixel_corr_pooled): a trend that is constant within a segment is removed from pixel and trace
        alike.  L > n_frames / 2 is one segment: the bits of None.  The traces of the same pass are not detrended."""
        # ---- everything that can be wrong with the arguments is a ValueError before the library or the GPU is touched ----
        shape = _check_shape(shape)
        halo = _check_halo(halo)
        n_frames = _check_n_frames(n_frames, shape, max_volume=MAX_VOLUME)
        if n_frames > MAX_FRAMES:
            raise ValueError('n_frames must be <= 2**31 - 1, not %d' % n_frames)
        self._seg = None
        if detrend_frames is not None:
            from .series import _Segments, _check_detrend_frames
            self._seg = _Segments(n_frames, _check_detrend_frames(detrend_frames, n_frames, shape))
        pixels = _roi_pixels(rois, shape)
        flat, inside = _support(pixels, shape, halo)
        self._coords = [np.stack([f // shape[1], f % shape[1]], 1).astype(np.int64) for f in flat]
        self._inside = inside
        counts, row_off, row_pix, row_roi = rois_to_csr(self._coords, shape)
        self._bounds = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
        self.halo, self.n_entries = halo, int(self._bounds[-1])
        own = [np.stack([p.astype(np.int64) // shape[1], p.astype(np.int64) % shape[1]], 1) for p in pixels]
        # slots of its own: an extractor alive at the same time keeps its own
        self._ext = ext = _LeadingExtractor('footprints_stage', self._accumulate, shape, n_frames, dtype, own, device=device,
                                            chunk_frames=chunk_frames, shifts=shifts, fine_shifts=fine_shifts, bidi=bidi)
        self.shape, self.n_frames, self.dtype, self.n_rois = shape, n_frames, ext.dtype, ext.n_rois
        self.chunk_frames, self.device, self.L = ext.chunk_frames, ext.device, ext.L
        torch = self._torch = ext._torch
        dev = self.device
        self._row_off = torch.from_numpy(row_off).to(dev)
        self._row_pix = torch.from_numpy(row_pix).to(dev)
        self._row_roi = torch.from_numpy(row_roi).to(dev)
        self._flags = torch.from_numpy(np.concatenate(inside).astype(np.int32)).to(dev)
        self._rows = len(row_roi)
        self._mom = torch.zeros((4, self.n_entries), dtype=torch.int64, device=dev)      # a, b, c_lo, c_hi: the kernel adds
        if self._seg is not None:        # pooled Cxx, Cxs per entry and Css per ROI: 16-byte {lo, hi} words; the segment's u, w
            self._pxx = torch.zeros((self.n_entries, 2), dtype=torch.int64, device=dev)
            self._pxs = torch.zeros((self.n_entries, 2), dtype=torch.int64, device=dev)
            self._pss = torch.zeros((self.n_rois, 2), dtype=torch.int64, device=dev)
            self._rmom = torch.empty((3, self.n_rois), dtype=torch.int64, device=dev)
        self._corr = None
        ext._constructed()               # again: the fills above belong to what its feed() waits for

    @property
    def fed(self):
        return self._ext.fed

    def _accumulate(self, fp, tc, t0, st):
        H, W = self.shape
        if self._seg is not None:        # cut at the segment boundaries; a segment that ends is folded, which leaves mom zero
            for k, m, _, ends in self._seg.cut(t0, tc):
                self._accumulate_frames(fp + k * H * W * 2, m, t0 + k, st)
                if ends is not None:
                    self.L.dc_roi_trace_moments(self._ext.sums.data_ptr() + 8 * ends[0], self.n_frames, self.n_rois, ends[1],
                                                self._rmom.data_ptr(), st)
                    self.L.dc_roi_pixel_fold_segment(self._mom.data_ptr(), self.n_entries, self._row_off.data_ptr(), self._row_roi.data_ptr(),
                                                     self._rows, self.n_rois, self._rmom.data_ptr(), ends[1], ends[2], self._pxx.data_ptr(),
                                                     self._pxs.data_ptr(), self._pss.data_ptr(), H, W, st)
            return
        self._accumulate_frames(fp, tc, t0, st)

    def _accumulate_frames(self, fp, tc, t0, st):
        H, W = self.shape
        ext = self._ext
        self.L.dc_roi_pixel_accumulate(fp, int(self.dtype == np.dtype(np.uint16)), tc, t0, self._row_off.data_ptr(),
                                       self._row_pix.data_ptr(), self._row_roi.data_ptr(), self._rows, self.n_rois,
                                       ext.sums.data_ptr(), self.n_frames, self._mom.data_ptr(), self.n_entries, H, W, st)

    def feed(self, frames):
        """The next frames of the recording: what RoiTraceExtractor.feed takes.  Per chunk dc_roi_trace_accumulate and then
        dc_roi_pixel_accumulate run on the same stream on the same frames."""
        self._ext.feed(frames)
        return self

    def support(self):
        """Per ROI the (k,2) int64 [y,x] of its support, in flat-index order."""
        return [c.copy() for c in self._coords]

    def inside(self):
        """Per ROI a bool (k,): the entry is one of the ROI's own pixels."""
        return [i.copy() for i in self._inside]

    def traces(self, kind='mean'):
        """RoiTraceExtractor.result(kind) of the same pass.  Fed the output of a series.TemporalBinner, these are the traces of the
        BINNED recording (n_frames // bin_frames samples of rounded means): a trace of every frame is another, unbinned pass."""
        return self._ext.result(kind)

    def sums_device(self):
        return self._ext.sums_device()

    def _split(self, flat):
        return [flat[self._bounds[r]:self._bounds[r + 1]] for r in range(self.n_rois)]

    def _corr_flat(self):
        if self._corr is None:
            torch, ext = self._torch, self._ext
            with torch.cuda.device(self.device):
                st = torch.cuda.current_stream(self.device).cuda_stream
                corr = torch.empty((self.n_entries,), dtype=torch.float32, device=self.device)
                if self._seg is not None:
                    self.L.dc_roi_pixel_corr_pooled(self._pxx.data_ptr(), self._pxs.data_ptr(), self._pss.data_ptr(), self.n_entries,
                                                    self._row_off.data_ptr(), self._row_roi.data_ptr(), self._rows, self.n_rois,
                                                    self._flags.data_ptr(), corr.data_ptr(), st)
                else:
                    rmom = torch.empty((3, self.n_rois), dtype=torch.int64, device=self.device)
                    self.L.dc_roi_trace_moments(ext.sums.data_ptr(), self.n_frames, self.n_rois, self.n_frames, rmom.data_ptr(), st)
                    self.L.dc_roi_pixel_corr(self._mom.data_ptr(), self.n_entries, self._row_off.data_ptr(), self._row_roi.data_ptr(),
                                             self._rows, self.n_rois, self._flags.data_ptr(), rmom.data_ptr(), self.n_frames,
                                             corr.data_ptr(), st)
            self._corr = corr.cpu().numpy()
        return self._corr

    def result(self, kind='corr'):
        """'corr': a list of R float32 arrays aligned with support(); 'moments': per ROI a dict of object arrays a, b, c of exact
        Python ints; 'coherence': float64 (R,), the mean of corr over every ROI's inside entries."""
        _check_kind(kind)
        if self.fed != self.n_frames:
            raise ValueError('result() after %d of %d frames' % (self.fed, self.n_frames))
        if kind == 'moments' and self._seg is not None:      # the pooled numerators, exact, with M: integers before any float
            from .series import _pooled_ints
            xx, xs = _pooled_ints(self._pxx.cpu().numpy()), _pooled_ints(self._pxs.cpu().numpy())
            ss = _pooled_ints(self._pss.cpu().numpy())
            return [dict(Cxx=x, Cxs=y, Css=ss[r], M=self._seg.M) for r, (x, y) in enumerate(zip(self._split(xx), self._split(xs)))]
        if kind == 'moments':
            m = self._mom.cpu().numpy()
            a, b = m[0].astype(object), m[1].astype(object)
            c = m[3].astype(object) * (1 << 64) + m[2].view(np.uint64).astype(object)
            return [dict(a=x, b=y, c=z) for x, y, z in zip(self._split(a), self._split(b), self._split(c))]
        corr = self._split(self._corr_flat())
        if kind == 'corr':
            return [c.copy() for c in corr]
        return np.array([c[i].astype(np.float64).mean() for c, i in zip(corr, self._inside)], np.float64)


def roi_footprints_device(dspath, rois, halo=2, source='series/raw', device=None, chunk_frames=None, shifts=None, fine_shifts=None,
                          bin_frames=None, detrend_frames=None, keep=None, bidi=0):
    """-> (corr, coords, inside) of `rois` (any form rois_to_csr takes) over `source` of a dataset file, streamed chunk by chunk:
    the recording is read once.  shifts / fine_shifts / bidi: as for extract_traces_device.  bin_frames: None, or an integer b in
    [1, 64]: the maps are those of the T // b rounded means of b consecutive corrected frames, correlated with the ROI traces of
    that binned recording (series.TemporalBinner; the trailing T % b frames are dropped, 1 gives what None gives).  detrend_frames: None, or an
    integer L in [2, 4096]: the correlations are pooled over segments of L frames (RoiFootprints); binning comes first and L counts
    binned frames.  Results at different L are not comparable with each other or with None.  keep: None, or a (T,) array of booleans
    (frames.flag_frames): the frames marked False are left out after bidi and the shifts and before binning and detrending, whose b
    and L then count kept frames; all True gives what None gives."""
    from .series import _check_detrend_frames
    _check_halo(halo)
    if detrend_frames is not None:
        _check_detrend_frames(detrend_frames)

    def reader_of(shape, n_frames, dtype, **kw):
        return RoiFootprints(shape, n_frames, dtype, rois, halo=halo, detrend_frames=detrend_frames, **kw)
    fp = _read_recording(dspath, source, reader_of, device, chunk_frames, shifts, fine_shifts, bidi, bin_frames, keep)
    return fp.result('corr'), fp.support(), fp.inside()
