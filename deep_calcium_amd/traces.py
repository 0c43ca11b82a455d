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

from .series import (_CHUNK_BYTES, _ShiftedChunks, _TwoSlotStage, _check_bidi, _check_device_frames, _check_known_shifts, _frame_dtype,
                     _open_series)

KINDS = ('sum', 'mean', 'zscore')
# Longest CSR row handed to the kernel: a longer ROI is cut into rows of this many pixels, so that one whole-image ROI among
# hundreds of small ones becomes hundreds of workgroups instead of one that walks it alone.  (The kernel itself takes rows
# of any length; 512 * 65535 < 2^31, so a row's sum over one frame fits int32.)
SEGMENT_PIXELS = 512
MAX_VOLUME = 1 << 46                  # DC_ROI_TRACE_MAX_VOLUME: T * H * W up to which the 128-bit z-score numerators fit


def _check_kind(kind):
    if kind not in KINDS:
        raise ValueError('trace kind %r is not one of %s' % (kind, ', '.join(KINDS)))


def _check_shape(shape):
    try:
        shape = tuple(int(v) for v in shape)
    except TypeError:
        raise ValueError('shape must be (H, W), not %r' % (shape,))
    if len(shape) != 2 or min(shape) < 1 or shape[0] * shape[1] > (1 << 30):
        raise ValueError('shape must be (H, W) with 1 <= H * W <= 2**30, not %r' % (shape,))
    return shape


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


class RoiTraceExtractor(object):
    """Owns the device state of one recording's ROI traces; feed() the frames in order, in chunks of any size, then result()."""

    def __init__(self, shape, n_frames, dtype, rois, device=None, chunk_frames=None, shifts=None, fine_shifts=None, bidi=0):
        """shifts: None, or the (n_frames, 2) integer (dy, dx) of every frame (numpy or a device tensor, e.g.
        MotionCorrector.shifts_device()): each chunk is moved by dc_motion_apply (fill 0) before its ROIs are summed.  Piecewise-rigid
        (n_frames, By, Bx, 2) block shifts (MotionCorrector.block_shifts_device()) are taken too: dc_motion_warp moves the chunk.
        fine_shifts: instead of shifts, the same shapes in sixteenths of a pixel (MotionCorrector.fine_shifts_device()): each
        chunk is interpolated by dc_motion_apply_sub / dc_motion_warp_sub (fill 0).
        bidi: the whole-pixel offset of the odd lines (motion.estimate_bidi_device), undone by dc_bidi_apply (fill 0) before the
        shift move; with no shifts it is the only move."""
        # ---- everything that can be wrong with the arguments is a ValueError before the library or the GPU is touched ----
        shape = _check_shape(shape)
        H, W = shape
        n_frames = int(n_frames)
        if n_frames < 1 or n_frames * H * W > MAX_VOLUME:
            raise ValueError('n_frames must be >= 1 with n_frames * H * W <= 2**46, not %d' % n_frames)
        self.dtype = _frame_dtype(dtype)
        areas, row_off, row_pix, row_roi = rois_to_csr(rois, shape)
        if chunk_frames is None:
            chunk_frames = max(1, _CHUNK_BYTES // (2 * H * W))
        chunk_frames = int(chunk_frames)
        if chunk_frames < 1:
            raise ValueError('chunk_frames must be >= 1, not %d' % chunk_frames)
        shifts, fine = _check_known_shifts(shifts, fine_shifts, n_frames, shape)
        bidi = _check_bidi(bidi, shape)
        self.shape, self.n_frames, self.areas = shape, n_frames, areas
        self.n_rois = len(areas)
        self.chunk_frames = min(chunk_frames, n_frames)
        self.fed = 0
        self._stage = None
        self._stage_tag = 'traces_stage'
        self._after_chunk = None

        import torch
        from . import net
        from ._lib import lib
        self._torch, self._net = torch, net
        self.L = lib()
        if not torch.cuda.is_available():
            from ._lib import DcunetError
            raise DcunetError('RoiTraceExtractor needs a GPU (there is no CPU fallback)')
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        if self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        dev = self.device
        self._areas = torch.from_numpy(areas).to(dev)
        self._row_off = torch.from_numpy(row_off).to(dev)
        self._row_pix = torch.from_numpy(row_pix).to(dev)
        self._row_roi = torch.from_numpy(row_roi).to(dev)
        self._rows = len(row_roi)
        # every chunk writes its own columns of every row, so the state is never cleared
        self.sums = torch.empty((self.n_rois, n_frames), dtype=torch.int64, device=dev)
        self._shifted = None if shifts is None and not bidi else _ShiftedChunks(torch, self.L, dev, shifts, (self.chunk_frames, H, W), fine,
                                                                                self.dtype == np.dtype(np.uint16), bidi)

    def _stream(self):
        return self._torch.cuda.current_stream(self.device)

    def _launch(self, fp, tc, t0, st):
        """The sums of one chunk (weighted.WeightedTraceExtractor: the weighted entry point instead)."""
        H, W = self.shape
        self.L.dc_roi_trace_accumulate(fp, int(self.dtype == np.dtype(np.uint16)), tc, t0, self._row_off.data_ptr(),
                                       self._row_pix.data_ptr(), self._row_roi.data_ptr(), self._rows, self.n_rois,
                                       self.sums.data_ptr(), self.n_frames, H, W, st)

    def _accumulate(self, fp, tc, st):
        def accumulate(fp, tc, t0):
            self._launch(fp, tc, t0, st)
            if self._after_chunk is not None:     # a second reader of the same frames, behind the sums (footprints.RoiFootprints)
                self._after_chunk(fp, tc, t0, st)
        if self._shifted is None:
            accumulate(fp, tc, self.fed)
        else:
            self._shifted.run(fp, tc, self.fed, st, accumulate)
        self.fed += tc

    def feed(self, frames):
        """The next frames of the recording, any t >= 1: a (t, H, W) numpy array or memmap of the recording's dtype (staged
        through two pinned slots, the upload of one chunk beside the kernel on the previous one), or a contiguous (t, H, W)
        torch.int16 tensor on the extractor's device holding the recording's bits (read in place, no staging; the signedness
        is the declared dtype's)."""
        on_device = not isinstance(frames, np.ndarray) and hasattr(frames, 'is_cuda') and hasattr(frames, 'data_ptr')
        if not on_device and not isinstance(frames, np.ndarray):
            raise ValueError('frames must be a numpy array (or memmap) or a CUDA tensor, not %s' % type(frames).__name__)
        if len(frames.shape) != 3 or tuple(frames.shape[1:]) != self.shape:
            raise ValueError('frames must be (t, %d, %d), not %r' % (self.shape + (tuple(frames.shape),)))
        if on_device:
            _check_device_frames(self._torch, frames, self.dtype, self.device, 'extractor')
        elif frames.dtype != self.dtype:
            raise ValueError('frames are %s, the recording was declared %s' % (frames.dtype, self.dtype))
        if frames.shape[0] < 1 or self.fed + frames.shape[0] > self.n_frames:
            raise ValueError('%d frames after %d fed: the recording was declared to have %d' %
                             (frames.shape[0], self.fed, self.n_frames))
        torch = self._torch
        with torch.cuda.device(self.device):
            main = self._stream()
            st = main.cuda_stream
            if on_device:
                self._accumulate(frames.data_ptr(), int(frames.shape[0]), st)
                frames.record_stream(main)
            else:
                if self._stage is None:          # names of its own: a SeriesSummarizer alive at the same time keeps its slots
                    H, W = self.shape
                    self._stage = _TwoSlotStage(torch, self._net, self.device, self._stage_tag, (self.chunk_frames, H, W))
                self._stage.run(frames, main, lambda fp, tc: self._accumulate(fp, tc, st))
        return self

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


def extract_traces_device(dspath, rois, kind='mean', source='series/raw', device=None, chunk_frames=None, shifts=None,
                          fine_shifts=None, bidi=0):
    """The (R,T) traces of `rois` (any form rois_to_csr takes) over `source` of a dataset file, streamed chunk by chunk: the
    recording is memory-mapped or sliced, never read whole.  shifts: the (T, 2) (dy, dx) of every frame, or its (T, By, Bx, 2) block
    shifts (motion.estimate_shifts_device), applied on the device on the way in.  fine_shifts: instead, either shape in sixteenths
    of a pixel (estimate_shifts_device(subpixel=True)): the frames are interpolated on the way in.  bidi: the offset of the odd lines
    (motion.estimate_bidi_device), undone on the way in before the shifts."""
    _check_kind(kind)
    _check_bidi(bidi)
    if shifts is not None and fine_shifts is not None:
        raise ValueError('give shifts= (whole pixels) or fine_shifts= (sixteenths of a pixel), not both')
    frames, close = _open_series(dspath, source)
    try:
        if len(frames.shape) != 3:
            raise ValueError('%s of %s is not a (T,H,W) recording: %r' % (source, dspath, tuple(frames.shape)))
        T = int(frames.shape[0])
        ext = RoiTraceExtractor(tuple(frames.shape[1:]), T, frames.dtype, rois, device=device, chunk_frames=chunk_frames,
                                shifts=shifts, fine_shifts=fine_shifts, bidi=bidi)
        for a in range(0, T, ext.chunk_frames):
            ext.feed(np.asarray(frames[a:a + ext.chunk_frames]))
        out = ext.result(kind)
    finally:
        frames = None                        # a view of the file mapping: released before the file is closed
        close()
    return out


def write_traces_dataset(path, traces, name, spikes=None):
    """A dataset file of the spikes model's schema (unet_1d_segmentation.py:182-187): the attribute `name`, `traces` (R,T) and,
    when given, `spikes` (R,T) as uint8.  HDF5 through hdf5_min.Writer; a path ending in .npz gets the same members instead."""
    traces = np.asarray(traces)
    if traces.ndim != 2 or traces.dtype.kind not in 'fiu':
        raise ValueError('traces must be a numeric (R,T) matrix, not %s %r' % (traces.dtype, traces.shape))
    if spikes is not None:
        spikes = np.asarray(spikes)
        if spikes.shape != traces.shape:
            raise ValueError('spikes are %r, traces %r' % (spikes.shape, traces.shape))
        spikes = spikes.astype(np.uint8)
    if str(path).endswith('.npz'):
        members = dict(traces=traces, name=np.array(str(name)))
        if spikes is not None:
            members['spikes'] = spikes
        np.savez(path, **members)
        return path
    from . import hdf5_min
    w = hdf5_min.Writer()
    w.attrs['name'] = str(name)
    w.create_dataset('traces', data=traces)
    if spikes is not None:
        w.create_dataset('spikes', data=spikes)
    w.save(path)
    return path
