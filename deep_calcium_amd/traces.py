"""ROI traces on the device: a recording (T,H,W) of 16-bit frames and the neurons' ROIs -> one fluorescence trace per ROI.

The reference's spikes model reads a `traces` matrix (no. ROIs, no. frames) and a `name` attribute from its dataset files
(models/spikes/unet_1d_segmentation.py:182-187) and normalises every trace as (traces - mean) / std along time (:158-167);
nothing in the reference makes that matrix from a recording and a mask.  Here the frames are streamed once through the
dc_roi_trace_* kernels (include/dcunet.h):

    kind      dtype     what
    sum       int64     the sum of the ROI's pixels in every frame                       (exact)
    mean      float32   sum / area                                                       (bit-equal to numpy's float64 divide)
    zscore    float32   (trace - mean over time) / population std over time              (exact numerators, <= 1 ulp)

    ext = RoiTraceExtractor((H, W), T, np.int16, rois)
    for chunk in chunks: ext.feed(chunk)          # numpy / memmap chunks, or an int16 CUDA tensor that is already resident
    traces = ext.result('mean')                   # (R, T)

    traces = extract_traces_device('dataset.hdf5', mask)          # mask: what UNet2DSummary.predict() returns
    write_traces_dataset('traces.hdf5', traces, name)             # the spikes model's schema

A trace that is constant in time (a single frame included) has a z-score of exactly 0 here; numpy divides 0 by 0 there, and
the reference's own asserts on the normalised traces then fail.

Importing this module needs neither torch nor the GPU; constructing a RoiTraceExtractor does (there is no CPU fallback).
"""
import numpy as np

from ._reader import _FrameReader, _check_shape, _read_recording

KINDS = ('sum', 'mean', 'zscore')
# Longest CSR row handed to the kernel: a longer ROI is cut into rows of this many pixels, so that one whole-image ROI among
# hundreds of small ones becomes hundreds of workgroups instead of one that walks it alone.  (The kernel itself takes rows
# of any length; 512 * 65535 < 2^31, so a row's sum over one frame fits int32.)
SEGMENT_PIXELS = 512
MAX_VOLUME = 1 << 46                  # DC_ROI_TRACE_MAX_VOLUME: T * H * W up to which the 128-bit z-score numerators fit


def _check_kind(kind):
    if kind not in KINDS:
        raise ValueError('trace kind %r is not one of %s' % (kind, ', '.join(KINDS)))


def _roi_pixels(rois, shape):
    """-> list of sorted, de-duplicated int32 arrays of flat pixel indices y * W + x, one per ROI."""
    H, W = shape
    if isinstance(rois, np.ndarray) and rois.ndim == 2:
        if rois.shape != shape:
            raise ValueError('the mask is %r, the frames are %r' % (tuple(rois.shape), shape))
        from .nf_metrics import mask_to_regions
        coords = mask_to_regions(rois)                       # 8-connected, raster label order
    elif isinstance(rois, np.ndarray) and rois.ndim == 3:
        if rois.shape[1:] != shape:
            raise ValueError('the mask stack is %r, the frames are %r' % (tuple(rois.shape), shape))
        coords = [np.argwhere(m != 0) for m in rois]
    elif isinstance(rois, (list, tuple)):
        coords = [r['coordinates'] if isinstance(r, dict) else r for r in rois]
    else:
        raise ValueError('rois must be a 2-D mask, an (n,H,W) stack, or a list of (k,2) [y,x] arrays or region dicts, not %s'
                         % type(rois).__name__)
    if len(coords) == 0:
        raise ValueError('no ROIs')
    out = []
    for i, c in enumerate(coords):
        c = np.asarray(c)
        if c.size == 0:
            raise ValueError('ROI %d is empty' % i)
        if c.ndim != 2 or c.shape[1] != 2 or c.dtype.kind not in 'iu':
            raise ValueError('ROI %d: coordinates must be a (k,2) integer array of [y,x], not %s %r' % (i, c.dtype, c.shape))
        c = c.astype(np.int64)
        if c.min() < 0 or c[:, 0].max() >= H or c[:, 1].max() >= W:
            raise ValueError('ROI %d has a coordinate outside the %d x %d image' % (i, H, W))
        out.append(np.unique(c[:, 0] * W + c[:, 1]).astype(np.int32))
    return out


def rois_to_csr(rois, shape):
    """ROIs -> (areas int32[R], row_off int32[S+1], row_pix int32[row_off[S]], row_roi int32[S]): the CSR rows of
    dc_roi_trace_accumulate, every ROI cut into rows of at most SEGMENT_PIXELS pixels (row_roi names the owner; it is
    non-decreasing).  `rois`: a 2-D mask (labelled like nf_metrics.mask_to_regions: 8-connected, raster order), an (n,H,W) stack
    of one mask per ROI (a dataset's masks/raw), a list of (k,2) [y,x] arrays, or a list of Neurofinder region dicts
    {'coordinates': [[y,x], ...]}.  Pixels are de-duplicated and sorted per ROI.  Host only."""
    shape = _check_shape(shape)
    pixels = _roi_pixels(rois, shape)
    areas = np.array([len(p) for p in pixels], np.int32)
    nseg = (areas.astype(np.int64) + SEGMENT_PIXELS - 1) // SEGMENT_PIXELS
    row_roi = np.repeat(np.arange(len(pixels), dtype=np.int32), nseg)
    lengths = np.concatenate([np.diff(np.append(np.arange(0, a, SEGMENT_PIXELS), a)) for a in areas.tolist()])
    if int(areas.sum(dtype=np.int64)) >= (1 << 31):
        raise ValueError('the ROIs list %d pixels in all: more than int32 offsets address' % areas.sum(dtype=np.int64))
    row_off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    row_pix = np.concatenate(pixels).astype(np.int32)
    return areas, row_off, row_pix, row_roi


class RoiTraceExtractor(_FrameReader):
    """Owns the device state of one recording's ROI traces; feed() the frames in order, in chunks of any size, then result()."""
    _stage_tag, _noun = 'traces_stage', 'extractor'

    def __init__(self, shape, n_frames, dtype, rois, device=None, chunk_frames=None, shifts=None, fine_shifts=None, bidi=0):
        """shifts: None, or the (n_frames, 2) integer (dy, dx) of every frame (numpy or a device tensor, e.g.
        MotionCorrector.shifts_device()): each chunk is moved by dc_motion_apply (fill 0) before its ROIs are summed.  Piecewise-rigid
        (n_frames, By, Bx, 2) block shifts (MotionCorrector.block_shifts_device()) are taken too: dc_motion_warp moves the chunk.
        fine_shifts: instead of shifts, the same shapes in sixteenths of a pixel (MotionCorrector.fine_shifts_device()): each
        chunk is interpolated by dc_motion_apply_sub / dc_motion_warp_sub (fill 0).
        bidi: the whole-pixel offset of the odd lines (motion.estimate_bidi_device), undone by dc_bidi_apply (fill 0) before the
        shift move; with no shifts it is the only move."""
        # ---- everything that can be wrong with the arguments is a ValueError before the library or the GPU is touched ----
        self._declare(shape, n_frames, dtype, chunk_frames, shifts, fine_shifts, bidi, max_volume=MAX_VOLUME)
        areas, row_off, row_pix, row_roi = rois_to_csr(rois, self.shape)
        self.areas, self.n_rois = areas, len(areas)

        torch = self._open(device, 'RoiTraceExtractor')
        dev = self.device
        self._areas = torch.from_numpy(areas).to(dev)
        self._row_off = torch.from_numpy(row_off).to(dev)
        self._row_pix = torch.from_numpy(row_pix).to(dev)
        self._row_roi = torch.from_numpy(row_roi).to(dev)
        self._rows = len(row_roi)
        # every chunk writes its own columns of every row, so the state is never cleared
        self.sums = torch.empty((self.n_rois, self.n_frames), dtype=torch.int64, device=dev)
        self._constructed()

    def _launch(self, fp, tc, t0, st):
        """The sums of one chunk (weighted.WeightedTraceExtractor: the weighted entry point instead)."""
        H, W = self.shape
        self.L.dc_roi_trace_accumulate(fp, self._unsigned, tc, t0, self._row_off.data_ptr(),
                                       self._row_pix.data_ptr(), self._row_roi.data_ptr(), self._rows, self.n_rois,
                                       self.sums.data_ptr(), self.n_frames, H, W, st)

    def _chunk(self, fp, tc, t0, st):
        self._launch(fp, tc, t0, st)

    def sums_device(self):
        """The (R, T) int64 sums where they lie, on the device, once every frame has been fed: what dff.TraceBaseline reads in
        place.  The extractor's own state: do not write to it."""
        if self.fed != self.n_frames:
            raise ValueError('sums_device() after %d of %d frames' % (self.fed, self.n_frames))
        return self.sums

    def areas_host(self):
        """The pixel count of every ROI, int32[R], on the host."""
        return self.areas.copy()

    def result(self, kind='mean'):
        """(R, T): int64 for 'sum', float32 for 'mean' and 'zscore'."""
        _check_kind(kind)
        if self.fed != self.n_frames:
            raise ValueError('result() after %d of %d frames' % (self.fed, self.n_frames))
        torch = self._torch
        if kind == 'sum':
            return self.sums.cpu().numpy()
        with torch.cuda.device(self.device):
            out = torch.empty((self.n_rois, self.n_frames), dtype=torch.float32, device=self.device)
            self.L.dc_roi_trace_finalize(self.sums.data_ptr(), self.n_frames, self._areas.data_ptr(), self.n_rois, self.n_frames,
                                         out.data_ptr() if kind == 'mean' else None,
                                         out.data_ptr() if kind == 'zscore' else None, self._stream().cuda_stream)
        return out.cpu().numpy()


class _LeadingExtractor(RoiTraceExtractor):
    """The extractor a second reader of the same chunks owns (footprints.RoiFootprints, roi_pairs.RoiPairCorr): staging slots
    under the owner's name, and the owner's launches then(fp, tc, t0, st) behind the sums of every chunk, on the same stream."""

    def __init__(self, stage_tag, then, *args, **kw):
        self._stage_tag, self._then = stage_tag, then
        super(_LeadingExtractor, self).__init__(*args, **kw)

    def _chunk(self, fp, tc, t0, st):
        self._launch(fp, tc, t0, st)
        self._then(fp, tc, t0, st)


def extract_traces_device(dspath, rois, kind='mean', source='series/raw', device=None, chunk_frames=None, shifts=None,
                          fine_shifts=None, bidi=0):
    """The (R,T) traces of `rois` (any form rois_to_csr takes) over `source` of a dataset file, streamed chunk by chunk: the
    recording is memory-mapped or sliced, never read whole.  shifts: the (T, 2) (dy, dx) of every frame, or its (T, By, Bx, 2) block
    shifts (motion.estimate_shifts_device), applied on the device on the way in.  fine_shifts: instead, either shape in sixteenths
    of a pixel (estimate_shifts_device(subpixel=True)): the frames are interpolated on the way in.  bidi: the offset of the odd lines
    (motion.estimate_bidi_device), undone on the way in before the shifts."""
    _check_kind(kind)
    def reader_of(shape, n_frames, dtype, **kw):
        return RoiTraceExtractor(shape, n_frames, dtype, rois, **kw)
    ext = _read_recording(dspath, source, reader_of, device, chunk_frames, shifts, fine_shifts, bidi)
    return ext.result(kind)


def write_traces_dataset(path, traces, name, spikes=None, extra=None):
    """A dataset file of the spikes model's schema (unet_1d_segmentation.py:182-187): the attribute `name`, `traces` (R,T) and,
    when given, `spikes` (R,T) as uint8.  HDF5 through hdf5_min.Writer; a path ending in .npz gets the same members instead.
    extra: None, or a dict of name -> numeric (R,T) array, written as further datasets in their own dtype (the `calcium` and
    `deconvolved` of deep_calcium_amd.deconv); with None the file is what it was before the argument existed, byte for byte."""
    traces = np.asarray(traces)
    if traces.ndim != 2 or traces.dtype.kind not in 'fiu':
        raise ValueError('traces must be a numeric (R,T) matrix, not %s %r' % (traces.dtype, traces.shape))
    if spikes is not None:
        spikes = np.asarray(spikes)
        if spikes.shape != traces.shape:
            raise ValueError('spikes are %r, traces %r' % (spikes.shape, traces.shape))
        spikes = spikes.astype(np.uint8)
    more = []
    for key, value in (extra or {}).items():
        value = np.asarray(value)
        if not isinstance(key, str) or not key or '/' in key or key in ('traces', 'spikes', 'name'):
            raise ValueError('extra: %r cannot name a further dataset' % (key,))
        if value.shape != traces.shape or value.dtype.kind not in 'fiu':
            raise ValueError('extra[%r] is %s %r, the traces are %r' % (key, value.dtype, value.shape, traces.shape))
        more.append((key, value))
    if str(path).endswith('.npz'):
        members = dict(traces=traces, name=np.array(str(name)))
        if spikes is not None:
            members['spikes'] = spikes
        members.update(more)
        np.savez(path, **members)
        return path
    from . import hdf5_min
    w = hdf5_min.Writer()
    w.attrs['name'] = str(name)
    w.create_dataset('traces', data=traces)
    if spikes is not None:
        w.create_dataset('spikes', data=spikes)
    for key, value in more:
        w.create_dataset(key, data=value)
    w.save(path)
    return path
