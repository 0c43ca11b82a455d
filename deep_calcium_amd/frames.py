"""Artefact frames: per-frame quality scores on the device, the rule that flags frames, and the stage that leaves them out.

A stimulation-light flash, a gated (dark) PMT frame, a z-jump: in such a frame all pixels move together, so a handful of them
pushes every pixel-pair and trace-pair correlation of the recording towards 1, becomes the `max` image and inflates `std`.  The
reference has no counterpart.  Here the frames are streamed once through dc_frame_moments / dc_frame_quality (include/dcunet.h,
"Frame quality"): per frame the exact sums over a rectangle, and from them

    kind      dtype     what
    moments   int64     (fed, 3): sum x, sum x^2, sum x * template over the rectangle     (exact)
    mean      float32   sum x / n                                                          (exact sum, one division)
    corr      float32   Pearson correlation of the frame with the template over the rectangle (exact numerators, <= 1 ulp)

    fq = FrameQuality((H, W), T, np.int16, template=tmpl)
    for chunk in chunks: fq.feed(chunk)
    keep = flag_frames(fq.result('mean'), fq.result('corr'))          # bool (T,): False for an artefact frame

    ff = FrameFilter((H, W), T, np.int16, keep)                        # in front of any reader, like TemporalBinner
    reader = RoiPairCorr((H, W), ff.n_out, np.int16, rois)
    for chunk in chunks:
        kept = ff.feed(chunk)
        if kept.shape[0]: reader.feed(kept)

The one-call functions that correlate (summarize_series_device, roi_footprints_device, roi_pair_corr_device, split_rois_device,
merge_rois_device) take keep= and do this themselves.  A trace needs every frame: extract_traces_device and dff_traces_device
take no keep=; hold_index(keep) patches their sums instead (sums[:, hold_index(keep)]).

Importing this module needs neither torch nor the GPU; constructing a FrameQuality or a FrameFilter does (there is no CPU fallback).
"""
import numpy as np

from ._reader import _FrameReader, _check_device_frames, _is_device_tensor, _read_recording

KINDS = ('moments', 'mean', 'corr')
MAX_PIXELS = 1 << 28                  # DC_FRAME_MAX_PIXELS: the pixels of the rectangle up to which the int64 sums hold


def _check_kind(kind):
    if kind not in KINDS:
        raise ValueError('frame quality kind %r is not one of %s' % (kind, ', '.join(KINDS)))


def _check_rect(rect, shape):
    """The `rect=` keyword: None (the whole frame) or ((y0, y1), (x0, x1)) as motion.valid_rectangle returns it -> (y0, y1, x0,
    x1).  Empty, outside the frame, or more than 2**28 pixels: ValueError.  Host only."""
    H, W = shape
    if rect is None:
        y0, y1, x0, x1 = 0, H, 0, W
    else:
        try:
            (y0, y1), (x0, x1) = rect
            ints = [v for v in (y0, y1, x0, x1) if isinstance(v, (int, np.integer)) and not isinstance(v, bool)]
        except (TypeError, ValueError):
            raise ValueError('rect must be ((y0, y1), (x0, x1)), not %r' % (rect,))
        if len(ints) != 4:
            raise ValueError('rect must be ((y0, y1), (x0, x1)) of integers, not %r' % (rect,))
        y0, y1, x0, x1 = (int(v) for v in ints)
        if y0 < 0 or x0 < 0 or y1 > H or x1 > W:
            raise ValueError('rect rows [%d, %d), columns [%d, %d) is outside the %d x %d frame' % (y0, y1, x0, x1, H, W))
        if y0 >= y1 or x0 >= x1:
            raise ValueError('rect rows [%d, %d), columns [%d, %d) is empty' % (y0, y1, x0, x1))
    if (y1 - y0) * (x1 - x0) > MAX_PIXELS:
        raise ValueError('the rectangle has %d pixels: limited to 2**28 (the int64 sums of a frame)' % ((y1 - y0) * (x1 - x0)))
    return y0, y1, x0, x1


def _check_keep(keep, n_frames=None):
    """The `keep=` keyword: a (n_frames,) array of booleans, True for a frame that stays -> a contiguous bool array.  The wrong
    length, or no frame kept: ValueError.  Host only."""
    a = np.asarray(keep)
    if a.ndim != 1 or a.dtype != np.bool_:
        raise ValueError('keep must be a one-dimensional array of booleans (True: the frame stays), not %s %r' % (a.dtype, a.shape))
    if n_frames is not None and a.shape[0] != n_frames:
        raise ValueError('keep has %d entries, the recording has %d frames' % (a.shape[0], n_frames))
    if not a.any():
        raise ValueError('keep keeps no frame')
    return np.ascontiguousarray(a)


def _mad_scale(v):
    med = np.median(v)
    return med, 1.4826 * np.median(np.abs(v - med))


def flag_frames(mean, corr=None, k=8.0):
    """The rule on the scores -> keep, a bool (T,) array, False for a flagged frame.  Float64 numpy on the host.  For a vector v,
    med = np.median(v) and s = 1.4826 * np.median(abs(v - med)) (the median absolute deviation, scaled to a standard deviation).
    A frame is dropped if abs(mean - med) > k * s; with corr, also if med_c - corr > k * s_c -- only a LOW correlation drops a
    frame, a frame that looks more like the template than most is no artefact.  k is a definition, like the merge threshold, not a
    measurement.  s == 0 (more than half of the values equal the median) flags EVERY frame that differs from the median: that is
    the rule taken literally, and a recording that regular has no noise to hide a difference in."""
    if isinstance(k, bool) or not isinstance(k, (int, float, np.integer, np.floating)) or not k > 0 or not np.isfinite(k):
        raise ValueError('k must be a finite number > 0, not %r' % (k,))
    m = np.asarray(mean, np.float64)
    if m.ndim != 1 or m.shape[0] < 1:
        raise ValueError('mean must be a (T,) vector with T >= 1, not %r' % (m.shape,))
    if not np.isfinite(m).all():
        raise ValueError('mean holds a value that is not finite')
    med, s = _mad_scale(m)
    keep = ~(np.abs(m - med) > float(k) * s)
    if corr is not None:
        c = np.asarray(corr, np.float64)
        if c.shape != m.shape:
            raise ValueError('corr must have the shape of mean, %r, not %r' % (m.shape, c.shape))
        if not np.isfinite(c).all():
            raise ValueError('corr holds a value that is not finite')
        med_c, s_c = _mad_scale(c)
        keep &= ~(med_c - c > float(k) * s_c)
    return keep


def hold_index(keep):
    """keep (T,) -> int64 (T,): for every frame the index of the latest kept frame at or before it, and the first kept frame for
    a leading run of dropped frames.  sums[:, hold_index(keep)] patches int64 trace sums (numpy, or a tensor with the index moved
    to its device) by holding the last good sample: no kernel."""
    keep = _check_keep(keep)
    kept = np.flatnonzero(keep).astype(np.int64)
    pos = np.searchsorted(kept, np.arange(keep.shape[0], dtype=np.int64), side='right') - 1
    return kept[np.maximum(pos, 0)]


class FrameQuality(_FrameReader):
    """Owns the per-frame sums of one recording; feed() the frames in order, in chunks of any size, then result().  Chunk
    boundaries never change a bit."""
    _stage_tag, _noun = 'fqual_stage', 'frame quality'

    def __init__(self, shape, n_frames, dtype, template=None, rect=None, shifts=None, fine_shifts=None, bidi=0, device=None, chunk_frames=None):
        """template: None, or the (H, W) image of the recording's dtype the frames are correlated with (motion.make_template's,
        MotionCorrector's), numpy or a torch.int16 tensor of its bits on the device; without one there is no 'corr'.
        rect: None (the whole frame) or ((y0, y1), (x0, x1)), what motion.valid_rectangle returns: the pixels every corrected
        frame really holds, at most 2**28.  shifts / fine_shifts / bidi: as for SeriesSummarizer, applied BEFORE the sums: the
        scores are those of the corrected frames."""
        # ---- everything that can be wrong with the arguments is a ValueError before the library or the GPU is touched ----
        self._declare(shape, n_frames, dtype, chunk_frames, shifts, fine_shifts, bidi)
        shape = self.shape
        self.rect = _check_rect(rect, shape)
        tmpl_on_device = template is not None and _is_device_tensor(template)
        if template is not None and not tmpl_on_device:
            template = np.asarray(template)
            if template.shape != shape or template.dtype != self.dtype:
                raise ValueError('template must be a %d x %d image of the recording\'s %s, not %s %r' % (shape + (self.dtype, template.dtype,
                                                                                                               tuple(template.shape))))
        elif tmpl_on_device and tuple(template.shape) != shape:
            raise ValueError('template must be a %d x %d image, not %r' % (shape + (tuple(template.shape),)))
        self.n_pixels = (self.rect[1] - self.rect[0]) * (self.rect[3] - self.rect[2])

        torch = self._open(device, 'FrameQuality')
        dev = self.device
        H, W = shape
        self._tmpl, self._tsums = None, None
        with torch.cuda.device(dev):
            if template is not None:
                if tmpl_on_device:
                    _check_device_frames(torch, template, self.dtype, dev, 'frame quality')
                    self._tmpl = template
                else:
                    self._tmpl = torch.from_numpy(np.ascontiguousarray(template).view(np.int16)).to(dev)
                # ta = sum tmpl, tb = sum tmpl^2 over the rectangle: the template as a chunk of one frame
                self._tsums = torch.empty((1, 3), dtype=torch.int64, device=dev)
                self.L.dc_frame_moments(self._tmpl.data_ptr(), self._unsigned, 1, None, H, W, self.rect[0], self.rect[1], self.rect[2], self.rect[3],
                                        self._tsums.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            # rows [0, fed) are written, each by the call that reads its frame: never cleared here
            self._moments = torch.empty((self.n_frames, 3), dtype=torch.int64, device=dev)
        self._constructed()

    def _chunk(self, fp, tc, t0, st):
        (H, W), (y0, y1, x0, x1) = self.shape, self.rect
        self.L.dc_frame_moments(fp, self._unsigned, tc, self._tmpl.data_ptr() if self._tmpl is not None else None, H, W, y0, y1, x0, x1,
                                self._moments.data_ptr() + 24 * t0, st)

    def result_device(self, kind):
        """result(kind) as a tensor on the device, for the frames fed so far."""
        _check_kind(kind)
        if kind == 'corr' and self._tmpl is None:
            raise ValueError("'corr' needs a template: FrameQuality(..., template=...)")
        torch = self._torch
        if kind == 'moments':
            return self._moments[:self.fed]
        with torch.cuda.device(self.device):
            mean = torch.empty((self.fed,), dtype=torch.float32, device=self.device)
            corr, ta, tb = None, 0, 0
            if self._tmpl is not None:
                corr = torch.empty((self.fed,), dtype=torch.float32, device=self.device)
                ta, tb = (int(v) for v in self._tsums.cpu().numpy()[0, :2])
            if self.fed:
                self.L.dc_frame_quality(self._moments.data_ptr(), self.fed, self.n_pixels, ta, tb, mean.data_ptr(),
                                        corr.data_ptr() if corr is not None else None, torch.cuda.current_stream(self.device).cuda_stream)
        return mean if kind == 'mean' else corr

    def result(self, kind):
        """'moments': int64 (fed, 3) = {sum x, sum x^2, sum x * template} per frame (the third 0 without a template); 'mean',
        'corr': float32 (fed,).  'corr' without a template is a ValueError."""
        return self.result_device(kind).cpu().numpy()


def frame_quality_device(dspath, template=None, rect=None, source='series/raw', device=None, chunk_frames=None, shifts=None, fine_shifts=None,
                         bidi=0):
    """-> (mean, corr or None), float32 (T,) each: the scores of every frame of `source` of a dataset file, streamed chunk by
    chunk through a FrameQuality; the recording is read once.  corr is None without a template."""
    def reader_of(shape, n_frames, dtype, **kw):
        return FrameQuality(shape, n_frames, dtype, template=template, rect=rect, **kw)
    fq = _read_recording(dspath, source, reader_of, device, chunk_frames, shifts, fine_shifts, bidi)
    return fq.result('mean'), (fq.result('corr') if template is not None else None)


class FrameFilter(_FrameReader):
    """Leaves frames out in front of the readers: the recording's frames in, the kept ones out, on the device (dc_frame_gather).
    Built like TemporalBinner: every reader takes the kept frames as it takes the raw ones, declared with n_out frames.

    n_out = keep.sum(); fed: frames consumed so far; emitted: frames written so far."""
    _stage_tag, _noun = 'ffilt_stage', 'frame filter'

    def __init__(self, shape, n_frames, dtype, keep, shifts=None, fine_shifts=None, bidi=0, device=None, chunk_frames=None):
        """keep: (n_frames,) booleans, True for a frame that stays (flag_frames); at least one.  shifts / fine_shifts / bidi: as for
        SeriesSummarizer, applied BEFORE the gather (dc_bidi_apply, then the shift move, fill 0): the rows of the tables are
        those of the recording's frames, not of the kept ones."""
        # ---- everything that can be wrong with the arguments is a ValueError before the library or the GPU is touched ----
        self._declare(shape, n_frames, dtype, chunk_frames, shifts, fine_shifts, bidi)
        self.keep = _check_keep(keep, self.n_frames)
        self._kept = np.flatnonzero(self.keep).astype(np.int32)
        self.n_out = int(self._kept.shape[0])
        self.emitted = 0

        torch = self._open(device, 'FrameFilter')
        self._kept_dev = torch.from_numpy(self._kept).to(self.device)      # the kept frames' indices in the recording, ascending
        self._constructed()

    def feed(self, frames):
        """The next frames of the recording, any t >= 1: what SeriesSummarizer.feed takes.  -> the kept ones among them: a
        contiguous (k, H, W) torch.int16 tensor on the device holding the bits of the recording's dtype, k >= 0.  It is a FRESH
        allocation every time, written on the current stream: no later feed touches it, and a reader fed on the same stream
        right away reads it after the kernels that wrote it.  A feed that keeps nothing moves nothing, upload and corrections
        included."""
        return super(FrameFilter, self).feed(frames)

    def _begin_feed(self, t):
        lo, hi = (int(v) for v in np.searchsorted(self._kept, (self.fed, self.fed + t)))
        out = self._torch.empty((hi - lo,) + self.shape, dtype=self._torch.int16, device=self.device)
        self._dst = out.data_ptr()           # where the next kept frame goes
        return out, hi > lo

    def _chunk(self, fp, tc, t0, st):
        H, W = self.shape
        a, b = (int(v) for v in np.searchsorted(self._kept, (t0, t0 + tc)))
        if b > a:
            idx = self._kept_dev[a:b] - t0                 # the positions within these tc frames
            self.L.dc_frame_gather(fp, tc, idx.data_ptr(), b - a, H, W, self._dst, st)
            self._dst += 2 * H * W * (b - a)
            self.emitted += b - a
