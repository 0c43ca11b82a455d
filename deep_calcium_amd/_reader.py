"""What every reader of a recording shares: the checks of its declaration, the device, feed() and the one-call driver.

A reader (series.SeriesSummarizer, traces.RoiTraceExtractor, frames.FrameQuality, ...) is declared with the recording's frame shape,
length and dtype and is then fed the frames in order, in chunks of any size.  _FrameReader holds everything about that which does
not depend on what the reader computes; a subclass adds its own argument checks and state, _chunk() -- the launches on one chunk --
and result().  _read_recording is the pass over a dataset file that every one-call function (summarize_series_device, ...) makes.

Importing this module needs neither torch nor the GPU.
"""
import numpy as np

from ._matrix import _is_device_tensor

MAX_FRAMES = 2147483647               # DC_SERIES_MAX_FRAMES: what the int64 state holds
_CHUNK_BYTES = 32 << 20               # default staging chunk: long enough to hide the launches, short enough to pin twice
_MAX_BLOCKS = 32                      # DC_MOTION_MAX_BLOCKS


def _frame_dtype(dtype):
    try:
        dt = np.dtype(dtype)
    except TypeError:
        raise ValueError('frames must be int16 or uint16, not %r' % (dtype,))
    if dt not in (np.dtype(np.int16), np.dtype(np.uint16)):
        raise ValueError('frames must be int16 or uint16, not %s' % dt)
    return dt


def _check_shape(shape):
    try:
        shape = tuple(int(v) for v in shape)
    except TypeError:
        raise ValueError('shape must be (H, W), not %r' % (shape,))
    if len(shape) != 2 or min(shape) < 1 or shape[0] * shape[1] > (1 << 30):
        raise ValueError('shape must be (H, W) with 1 <= H * W <= 2**30, not %r' % (shape,))
    return shape


def _check_n_frames(n_frames, shape, max_frames=None, max_volume=None):
    """The declared length against the reader's own limit: max_volume bounds n_frames * H * W (the ROI readers), max_frames
    n_frames itself; with neither it only has to be positive."""
    n_frames = int(n_frames)
    if max_volume is not None:
        if n_frames < 1 or n_frames * shape[0] * shape[1] > max_volume:
            raise ValueError('n_frames must be >= 1 with n_frames * H * W <= 2**%d, not %d' % (max_volume.bit_length() - 1, n_frames))
    elif max_frames is not None:
        if not 1 <= n_frames <= max_frames:
            raise ValueError('n_frames must be in [1, %d], not %d' % (max_frames, n_frames))
    elif n_frames < 1:
        raise ValueError('n_frames must be >= 1, not %d' % n_frames)
    return n_frames


def _check_chunk_frames(chunk_frames, shape):
    """The `chunk_frames=` keyword: None is the default staging chunk of _CHUNK_BYTES."""
    if chunk_frames is None:
        chunk_frames = max(1, _CHUNK_BYTES // (2 * shape[0] * shape[1]))
    chunk_frames = int(chunk_frames)
    if chunk_frames < 1:
        raise ValueError('chunk_frames must be >= 1, not %d' % chunk_frames)
    return chunk_frames


def _shifts_shape_ok(shape, n_frames, frame_shape):
    """(n_frames, 2): one rigid (dy, dx) per frame; (n_frames, By, Bx, 2): one per block of a grid that fits the frame."""
    shape = tuple(shape)
    if shape == (n_frames, 2):
        return True
    if len(shape) != 4 or shape[0] != n_frames or shape[3] != 2:
        return False
    limit = (_MAX_BLOCKS, _MAX_BLOCKS) if frame_shape is None else (min(_MAX_BLOCKS, frame_shape[0]), min(_MAX_BLOCKS, frame_shape[1]))
    return 1 <= shape[1] <= limit[0] and 1 <= shape[2] <= limit[1]


def _check_shifts(shifts, n_frames, frame_shape=None, name='shifts'):
    """The `shifts=` keyword of SeriesSummarizer / RoiTraceExtractor: None, an (n_frames, 2) integer numpy array of (dy, dx) rows
    (-> contiguous int32) or an (n_frames, 2) integer tensor (checked, returned as it is); or the piecewise-rigid
    (n_frames, By, Bx, 2) block shifts of either kind, By and Bx in [1, 32] and no more blocks than pixels.  `fine_shifts=`
    (name='fine_shifts': sixteenths of a pixel) is held to the same checks.  Host only."""
    if shifts is None:
        return None
    what = '%s must be an integer (n_frames, 2) = (%d, 2) array of (dy, dx), or (%d, By, Bx, 2) block shifts with By, Bx in [1, %d]' \
        % (name, n_frames, n_frames, _MAX_BLOCKS)
    if _is_device_tensor(shifts):
        if not _shifts_shape_ok(shifts.shape, n_frames, frame_shape) or shifts.dtype.is_floating_point or shifts.dtype.is_complex:
            raise ValueError('%s, not %s %r' % (what, shifts.dtype, tuple(shifts.shape)))
        return shifts
    a = np.asarray(shifts)
    if not _shifts_shape_ok(a.shape, n_frames, frame_shape) or a.dtype.kind not in 'iu':
        raise ValueError('%s, not %s %r' % (what, a.dtype, tuple(a.shape)))
    if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
        raise ValueError('%s must fit int32' % name)
    return np.ascontiguousarray(a.astype(np.int32))


def _check_one_table(shifts, fine_shifts):
    if shifts is not None and fine_shifts is not None:
        raise ValueError('give shifts= (whole pixels) or fine_shifts= (sixteenths of a pixel), not both')


def _check_known_shifts(shifts, fine_shifts, n_frames, frame_shape):
    """`shifts=` and `fine_shifts=` of a consumer of known shifts -> (the checked table or None, whether it is fine).  Giving both
    is a ValueError.  Host only."""
    _check_one_table(shifts, fine_shifts)
    if fine_shifts is not None:
        return _check_shifts(fine_shifts, n_frames, frame_shape, name='fine_shifts'), True
    return _check_shifts(shifts, n_frames, frame_shape), False


def _check_bidi(bidi, shape=None):
    """The `bidi=` keyword of MotionCorrector and every reader of known shifts: the whole-pixel offset the odd lines are moved by
    before anything else reads a frame (dc_bidi_apply), 0 for none.  An integer that keeps a column of the odd lines, |bidi| < W.
    Host only."""
    if isinstance(bidi, bool) or not isinstance(bidi, (int, np.integer)):
        raise ValueError('bidi must be an integer (the whole-pixel offset of the odd lines, 0 for none), not %r' % (bidi,))
    p = int(bidi)
    if not -2 ** 31 <= p < 2 ** 31:
        raise ValueError('bidi must fit int32, not %d' % p)
    if shape is not None and abs(p) >= shape[1]:
        raise ValueError('bidi = %d leaves no column of the odd lines of a %d x %d frame: |bidi| < W' % (p, shape[0], shape[1]))
    return p


def _check_device_frames(torch, frames, dtype, device, owner):
    """A feed() argument that is a tensor: the recording's bits as a contiguous torch.int16 tensor on `device`."""
    if frames.dtype != torch.int16:
        raise ValueError('a device tensor must be torch.int16 (the bits of the %s frames), not %s' % (dtype, frames.dtype))
    if not frames.is_cuda or frames.device != device:
        raise ValueError('the tensor is on %s, the %s on %s' % (frames.device, owner, device))
    if not frames.is_contiguous():
        raise ValueError('a device tensor must be contiguous')


def _open_device(device, name):
    """-> (torch, net, the library, the torch.device with its index): where host-only ends.  `name` needs a GPU."""
    import torch
    from . import net
    from ._lib import lib
    L = lib()
    if not torch.cuda.is_available():
        from ._lib import DcunetError
        raise DcunetError('%s needs a GPU (there is no CPU fallback)' % name)
    device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    return torch, net, L, device


class _ShiftedChunks(object):
    """Known shifts applied on the way in (fill 0): the int32 (n_frames, 2) table on the device (dc_motion_apply) or the
    (n_frames, By, Bx, 2) block shifts (dc_motion_warp) and one scratch chunk the accumulate kernels read instead of the staged
    frames.  Frame `fed + i` of the recording gets row `fed + i`.  fine: the table holds fine shifts (sixteenths of a pixel), the
    frames are interpolated (dc_motion_apply_sub, dc_motion_warp_sub: they are told the signedness).  bidi != 0: the odd lines
    are moved by it first (dc_bidi_apply, into a scratch chunk of its own); with shifts=None that is the only move."""

    def __init__(self, torch, L, device, shifts, shape, fine=False, unsigned=0, bidi=0):
        self._L, self.shape, self.fine, self._uns, self.bidi = L, shape, fine, int(unsigned), int(bidi)
        self.shifts, self.blocks = None, None
        if shifts is not None:
            if isinstance(shifts, np.ndarray):
                shifts = torch.from_numpy(shifts)
            self.shifts = shifts.to(device=device, dtype=torch.int32).contiguous()
            self.blocks = tuple(int(v) for v in self.shifts.shape[1:3]) if self.shifts.dim() == 4 else None
        self.scratch = torch.empty(shape, dtype=torch.int16, device=device)
        self._lines = torch.empty(shape, dtype=torch.int16, device=device) if self.bidi and self.shifts is not None else None

    def run(self, fp, tc, fed, st, launch):
        """launch(pointer to corrected frames, count, first frame, st) for the tc frames at fp, a scratch chunk at a time."""
        C, H, W = self.shape
        for a in range(0, tc, C):
            n = min(C, tc - a)
            src = fp + 2 * a * H * W
            if self.bidi:
                dst = self.scratch if self.shifts is None else self._lines
                self._L.dc_bidi_apply(src, n, self.bidi, H, W, 0, dst.data_ptr(), st)
                src = dst.data_ptr()
            if self.shifts is None:
                pass
            elif self.fine and self.blocks is None:
                self._L.dc_motion_apply_sub(src, self._uns, n, self.shifts.data_ptr() + 8 * (fed + a), H, W, 0,
                                            self.scratch.data_ptr(), st)
            elif self.fine:
                By, Bx = self.blocks
                self._L.dc_motion_warp_sub(src, self._uns, n, self.shifts.data_ptr() + 8 * By * Bx * (fed + a), By, Bx, H, W, 0,
                                           self.scratch.data_ptr(), st)
            elif self.blocks is None:
                self._L.dc_motion_apply(src, n, self.shifts.data_ptr() + 8 * (fed + a), H, W, 0,
                                        self.scratch.data_ptr(), st)
            else:
                By, Bx = self.blocks
                self._L.dc_motion_warp(src, n, self.shifts.data_ptr() + 8 * By * Bx * (fed + a), By, Bx, H, W, 0,
                                       self.scratch.data_ptr(), st)
            launch(self.scratch.data_ptr(), n, fed + a, st)


class _TwoSlotStage(object):
    """Two pinned host slots and two device slots of `shape` = (C, H, W) int16: the H2D copy of chunk k + 1 (copy stream) runs
    beside the kernels on chunk k (the caller's stream); events hand the slots back and forth.  The pinned slots are cached by
    name (net._pinned): every user passes a `tag` of its own, so two users alive at once never share a slot."""

    def __init__(self, torch, net, device, tag, shape):
        self._torch, self.chunk_frames = torch, int(shape[0])
        self._host = [net._pinned('%s%d' % (tag, k), shape, torch.int16, entry=True) for k in range(2)]
        self._dev = [torch.empty(shape, dtype=torch.int16, device=device) for _ in range(2)]
        with torch.cuda.device(device):
            self._copy_stream = torch.cuda.Stream(device=device)
        self._read = [None, None]         # event behind the last kernel that read device slot k
        self._slot = 0

    def run(self, frames, main, launch):
        """Cuts `frames` (numpy, 16-bit) into chunks, uploads each and calls launch(device pointer, frames in the chunk), which
        enqueues the chunk's kernels on `main`.  Called with the device current."""
        torch = self._torch
        for a in range(0, frames.shape[0], self.chunk_frames):
            part = frames[a:a + self.chunk_frames]
            tc, k = part.shape[0], self._slot
            self._slot ^= 1
            host, dev = self._host[k], self._dev[k]
            if host[1] is not None:
                host[1].synchronize()                  # the copy that last read this pinned slot has finished
            host[0].numpy()[:tc] = part.view(np.int16)         # same bits; the kernels are told the signedness
            with torch.cuda.stream(self._copy_stream):
                if self._read[k] is not None:
                    self._copy_stream.wait_event(self._read[k])      # the kernels on chunk k - 2 are done with the slot
                dev[:tc].copy_(host[0][:tc], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(self._copy_stream)
            host[1] = ev
            main.wait_event(ev)
            launch(dev.data_ptr(), tc)
            done = torch.cuda.Event()
            done.record(main)
            self._read[k] = done


class _FrameReader(object):
    """A reader that is fed the frames of a recording in order.  A subclass's __init__ calls _declare() (host only), makes its own
    checks, calls _open() (the device), allocates its state and ends with _constructed(); it defines _chunk() and result().

    _stage_tag names the reader's pinned staging slots (cached by name: two readers alive at once never share one); _noun is what
    the reader is called where a tensor lies on another device."""
    _stage_tag = None
    _noun = None

    def _declare(self, shape, n_frames, dtype, chunk_frames, shifts=None, fine_shifts=None, bidi=0, max_frames=MAX_FRAMES, max_volume=None):
        """Everything that can be wrong with the declaration is a ValueError before torch or the library is imported.  n_frames
        None (motion.BidiEstimator): a reader of no declared length."""
        self.shape = _check_shape(shape)
        self.n_frames = None if n_frames is None else _check_n_frames(n_frames, self.shape, max_frames, max_volume)
        self.dtype = _frame_dtype(dtype)
        self.chunk_frames = _check_chunk_frames(chunk_frames, self.shape)
        self._known = (None, False, 0)
        if self.n_frames is not None:
            self.chunk_frames = min(self.chunk_frames, self.n_frames)
            self._known = _check_known_shifts(shifts, fine_shifts, self.n_frames, self.shape) + (_check_bidi(bidi, self.shape),)
        self._unsigned = int(self.dtype == np.dtype(np.uint16))
        self.fed = 0
        self._stage = self._shifted = self._ready = None

    def _open(self, device, name):
        """The device: torch, the library, the normalised device, and the corrections _declare() checked.  -> torch."""
        torch, self._net, self.L, self.device = _open_device(device, name)
        self._torch = torch
        shifts, fine, bidi = self._known
        if shifts is not None or bidi:
            self._shifted = _ShiftedChunks(torch, self.L, self.device, shifts, (self.chunk_frames,) + self.shape, fine, self._unsigned, bidi)
        return torch

    def _stream(self):
        return self._torch.cuda.current_stream(self.device)

    def _constructed(self):
        """The last call of a constructor, on the stream it ran on: an event behind everything it enqueued there (the fills of
        torch.zeros / torch.full, a kernel).  feed() waits for it on its own stream, so a reader may be fed on another stream
        than the one it was made on.  The owner of a _LeadingExtractor calls it again once its own state is made."""
        with self._torch.cuda.device(self.device):
            self._ready = self._torch.cuda.Event()
            self._ready.record(self._stream())

    def _check_frames(self, frames):
        """The argument of a feed(): type, shape and dtype against the declaration -> whether it lies on the device."""
        on_device = _is_device_tensor(frames)
        if not on_device and not isinstance(frames, np.ndarray):
            raise ValueError('frames must be a numpy array (or memmap) or a CUDA tensor, not %s' % type(frames).__name__)
        if len(frames.shape) != 3 or tuple(frames.shape[1:]) != self.shape:
            raise ValueError('frames must be (t, %d, %d), not %r' % (self.shape + (tuple(frames.shape),)))
        if on_device:
            _check_device_frames(self._torch, frames, self.dtype, self.device, self._noun)
        elif frames.dtype != self.dtype:
            raise ValueError('frames are %s, the recording was declared %s' % (frames.dtype, self.dtype))
        return on_device

    def _staged(self):
        """The two-slot stage of host frames, made on first use: a reader fed device tensors only never pins memory."""
        if self._stage is None:
            self._stage = _TwoSlotStage(self._torch, self._net, self.device, self._stage_tag, (self.chunk_frames,) + self.shape)
        return self._stage

    def _begin_feed(self, t):
        """Called once per feed(), with the device current, before the first chunk of its t frames -> (what feed() returns,
        whether these frames have to be read at all).  The stages that return frames allocate them here."""
        return self, True

    def _chunk(self, fp, tc, t0, st):
        """The launches on the tc corrected frames at device pointer fp, frames [t0, t0 + tc) of the recording, on stream st."""
        raise NotImplementedError

    def feed(self, frames):
        """The next frames of the recording, any t >= 1: a (t, H, W) numpy array or memmap of the recording's dtype (staged
        through two pinned slots, the upload of one chunk beside the kernels on the previous one), or a contiguous (t, H, W)
        torch.int16 tensor on the reader's device holding the recording's bits (read in place, no staging; the signedness is
        the declared dtype's)."""
        on_device = self._check_frames(frames)
        t = int(frames.shape[0])
        if t < 1 or self.fed + t > self.n_frames:
            raise ValueError('%d frames after %d fed: the recording was declared to have %d' % (t, self.fed, self.n_frames))
        with self._torch.cuda.device(self.device):
            main = self._stream()
            main.wait_event(self._ready)                # the constructor's fills and launches, on whichever stream it ran
            st = main.cuda_stream
            out, needed = self._begin_feed(t)

            def consume(fp, tc):
                if self._shifted is None:
                    self._chunk(fp, tc, self.fed, st)
                else:
                    self._shifted.run(fp, tc, self.fed, st, self._chunk)
                self.fed += tc
            if not needed:
                self.fed += t
            elif on_device:
                consume(frames.data_ptr(), t)
                frames.record_stream(main)
            else:
                self._staged().run(frames, main, consume)
        return out


def _read_recording(dspath, source, reader_of, device=None, chunk_frames=None, shifts=None, fine_shifts=None, bidi=0, bin_frames=None,
                    keep=None):
    """The pass of the one-call functions: `source` of the dataset file `dspath`, memory-mapped or sliced, is fed in chunk_frames
    slices to reader_of(shape, n_frames, dtype, **kw) -> the reader, fed.  keep puts a frames.FrameFilter in front of it and
    bin_frames a series.TemporalBinner behind that; the reader is then declared with the frames that reach it, and the corrections
    (shifts / fine_shifts / bidi) are in the kw of whichever stage comes first, the reader's only if it is alone.  A binned pass
    without keep does not read the trailing frames that close no bin.  reader_of may return None: nothing is read then.  The
    checks that need no file come before it is opened, those that need the recording's length before the GPU is touched."""
    from .series import TemporalBinner, _check_bin_frames, _open_recording
    _check_one_table(shifts, fine_shifts)
    _check_bidi(bidi)
    if bin_frames is not None:
        _check_bin_frames(bin_frames)
    if keep is not None:
        from .frames import FrameFilter, _check_keep
        keep = _check_keep(keep)
    frames, close = _open_recording(dspath, source)
    try:
        used = n = int(frames.shape[0])
        shape, dtype = tuple(int(v) for v in frames.shape[1:]), frames.dtype
        kw = dict(device=device, chunk_frames=chunk_frames, shifts=shifts, fine_shifts=fine_shifts, bidi=bidi)
        stages = []
        if keep is not None:
            keep = _check_keep(keep, n)
            if bin_frames is not None:
                _check_bin_frames(bin_frames, int(keep.sum()))             # b counts kept frames
            stages.append(FrameFilter(shape, n, dtype, keep, **kw))
            n, kw = stages[-1].n_out, dict(device=stages[-1].device, chunk_frames=chunk_frames)
        if bin_frames is not None:
            stages.append(TemporalBinner(shape, n, dtype, bin_frames=bin_frames, **kw))
            if keep is None:
                used = stages[-1].n_out * stages[-1].bin_frames          # the trailing frames close no bin: not read
            n, kw = stages[-1].n_out, dict(device=stages[-1].device, chunk_frames=chunk_frames)
        reader = reader_of(shape, n, dtype, **kw)
        if reader is None:
            return None
        stages.append(reader)
        step = stages[0].chunk_frames
        for a in range(0, used, step):
            part = np.asarray(frames[a:min(a + step, used)])
            for stage in stages[:-1]:
                part = stage.feed(part)
                if not part.shape[0]:
                    break
            else:
                reader.feed(part)
        return reader
    finally:
        frames = None                        # a view of the file mapping: released before the file is closed
        close()
