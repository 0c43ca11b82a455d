"""Series summaries on the device: a recording (T,H,W) of 16-bit frames -> the (H,W) image the network segments.

The reference computes `series/mean` and `series/max` on the host while it builds a dataset (datasets/nf.py:121-130) and
leaves every other summary to the user's `series_summary_func` (unet_2d_summary.py:227-241 is the default).  Here the frames
are streamed once through the dc_series_* kernels (include/dcunet.h):

    kind      dtype     what
    mean16    float16   the reference's stored mean: accumulated in float16, one rounding per frame   (bit-exact)
    max16     int16     the reference's stored max: from 0, saturated at 32767                        (exact)
    mean      float32   sum / T                                        (exact sum, <= 1 ulp)
    max       float32   the true maximum                               (exact)
    std       float32   population standard deviation over time        (exact numerator, <= 1 ulp)
    corr      float32   mean Pearson correlation with the 8 neighbours (exact numerators, abs. error < 1e-14)

    summ = SeriesSummarizer((H, W), T, np.int16, kinds=('mean', 'corr'))
    for chunk in chunks: summ.feed(chunk)
    img = summ.result('corr')

    UNet2DSummary(series_summary_func=functools.partial(summarize_series_device, kind='corr'))

TemporalBinner (dc_series_bin_time) goes in front of any reader: the exact rounded means of b <= 64 consecutive frames, streamed,
so that what is correlated is a transient and not the pixel noise of single frames (bin_frames= of the one-call functions).

detrend_frames=L (SeriesSummarizer, and RoiFootprints / RoiPairCorr, which share detrend_plan): `std` and `corr` are formed from
centred moments pooled over segments of L frames (dc_series_fold_segment, dc_series_finalize_pooled), exact integers until the last
step, so that bleaching and drift common to all pixels do not push every correlation towards 1.  Piecewise-constant detrending: a
trend inside a segment stays; results at different L are not comparable with each other or with None.

Importing this module needs neither torch nor the GPU; constructing a SeriesSummarizer does (there is no CPU fallback).
"""
import numpy as np

# the checks and constants that moved to _reader stay importable from here
from ._reader import MAX_FRAMES, _CHUNK_BYTES, _check_bidi, _check_known_shifts, _check_shifts, _frame_dtype  # noqa: F401
from ._reader import _FrameReader, _read_recording

KINDS = ('mean16', 'max16', 'mean', 'max', 'std', 'corr')
MAX_BIDI = 16                         # DC_BIDI_MAX_OFFSET: the largest radius of the scan-phase search


def _check_kind(kind, kinds=KINDS):
    if kind not in KINDS:
        raise ValueError('summary kind %r is not one of %s' % (kind, ', '.join(KINDS)))
    if kind not in kinds:
        raise ValueError('summary kind %r was not requested (kinds=%r)' % (kind, tuple(kinds)))


MIN_DETREND_FRAMES = 2
MAX_DETREND_FRAMES = 4096             # DC_DETREND_MAX_FRAMES: the frames of one detrending segment
MAX_DETREND_VOLUME = 1 << 46          # M * H * W up to which the pooled 128-bit numerators fit (csrc/detrend_math.h)


def detrend_plan(T, L):
    """The segments of a recording of T frames detrended with `detrend_frames=L` -> [(t_start, len, mult)]: n = max(1, T // L)
    segments, n - 1 of L frames and a last one of L_last = T - (n - 1) L frames (L <= L_last < 2 L); T < 2 L: one segment of T
    frames.  mult = M / len with M = L * L_last (M = T when n == 1): L_last for a full segment, L for the last, 1 alone.  Host only."""
    T, L = int(T), int(L)
    if T < 1 or L < 1:
        raise ValueError('detrend_plan(T = %d, L = %d): both must be >= 1' % (T, L))
    n = max(1, T // L)
    if n == 1:
        return [(0, T, 1)]
    last = T - (n - 1) * L
    return [(s * L, L, last) for s in range(n - 1)] + [((n - 1) * L, last, L)]


def _check_detrend_frames(detrend_frames, n_frames=None, shape=None):
    """The `detrend_frames=` keyword: an integer L in [2, MAX_DETREND_FRAMES]; with the declared n_frames (and the frame shape)
    M * H * W <= 2**46, M = L * L_last of detrend_plan (M = n_frames for one segment).  Host only."""
    if isinstance(detrend_frames, bool) or not isinstance(detrend_frames, (int, np.integer)):
        raise ValueError('detrend_frames must be an integer in [%d, %d], not %r' % (MIN_DETREND_FRAMES, MAX_DETREND_FRAMES, detrend_frames))
    L = int(detrend_frames)
    if not MIN_DETREND_FRAMES <= L <= MAX_DETREND_FRAMES:
        raise ValueError('detrend_frames must be in [%d, %d], not %d' % (MIN_DETREND_FRAMES, MAX_DETREND_FRAMES, L))
    if n_frames is not None and shape is not None:
        plan = detrend_plan(n_frames, L)
        M = plan[0][1] * plan[0][2]
        if M * shape[0] * shape[1] > MAX_DETREND_VOLUME:
            raise ValueError('detrend_frames = %d on %d frames of %d x %d: M * H * W = %d * %d is limited to 2**46'
                             % (L, n_frames, shape[0], shape[1], M, shape[0] * shape[1]))
    return L


class _Segments(object):
    """Where a reader in detrend mode stands: cut(t0, tc) yields (offset in the chunk, frames, frame within the segment, the
    segment (t_start, len, mult) when the piece ends it, else None) for the frames [t0, t0 + tc) of the recording."""

    def __init__(self, n_frames, L):
        self.plan = detrend_plan(n_frames, L)
        self.L, self.n, self.n_frames = L, len(self.plan), n_frames
        self.M = self.plan[0][1] * self.plan[0][2]
        self.last = self.plan[-1][1]

    def cut(self, t0, tc):
        k = 0
        while k < tc:
            s = min((t0 + k) // self.L, self.n - 1)
            start, length, _ = self.plan[s]
            m = min(tc - k, start + length - (t0 + k))
            yield k, m, t0 + k - start, (self.plan[s] if t0 + k + m == start + length else None)
            k += m


def _pooled_ints(words):
    """int64 (..., 2) {lo, hi} pooled words -> an object array of exact Python ints, hi * 2^64 + lo."""
    return words[..., 1].astype(object) * (1 << 64) + words[..., 0].view(np.uint64).astype(object)


class SeriesSummarizer(_FrameReader):
    """Owns the device state of one recording's summaries; feed() the frames in order, in chunks of any size, then result()."""
    _stage_tag, _noun = 'series_stage', 'summarizer'

    def __init__(self, shape, n_frames, dtype, device=None, chunk_frames=None, kinds=KINDS, shifts=None, fine_shifts=None, detrend_frames=None,
                 bidi=0):
        """shifts: None, or the (n_frames, 2) integer (dy, dx) of every frame (numpy or a device tensor, e.g.
        MotionCorrector.shifts_device()): each chunk is moved by dc_motion_apply (fill 0) before it is summarised.  Piecewise-rigid
        (n_frames, By, Bx, 2) block shifts (MotionCorrector.block_shifts_device()) are taken too: dc_motion_warp moves the chunk.
        fine_shifts: instead of shifts, the same shapes in sixteenths of a pixel (MotionCorrector.fine_shifts_device()): each
        chunk is interpolated by dc_motion_apply_sub / dc_motion_warp_sub (fill 0).
        bidi: the whole-pixel offset of the odd lines (motion.estimate_bidi_device), undone by dc_bidi_apply (fill 0) before the
        shift move; with no shifts it is the only move.
        detrend_frames: None, or an integer L in [2, 4096]: `std` and `corr` are formed from centred moments pooled over the
        segments of detrend_plan(n_frames, L) (dc_series_fold_segment at every segment's end, dc_series_finalize_pooled), which
        removes every trend that is constant within a segment; `mean` and `max` are those of the whole recording; `mean16` /
        `max16` are not served.  L > n_frames / 2 is one segment: the `corr` bits of None."""
        # ---- everything that can be wrong with the arguments is a ValueError before the library or the GPU is touched ----
        self._declare(shape, n_frames, dtype, chunk_frames, shifts, fine_shifts, bidi)
        kinds = (kinds,) if isinstance(kinds, str) else tuple(kinds)
        if not kinds:
            raise ValueError('kinds is empty')
        for k in kinds:
            _check_kind(k)
        self._seg = None
        if detrend_frames is not None:
            self._seg = _Segments(self.n_frames, _check_detrend_frames(detrend_frames, self.n_frames, self.shape))
            if 'mean16' in kinds or 'max16' in kinds:
                raise ValueError('mean16 / max16 are the stored summaries of the whole recording: not served with detrend_frames')
        self.kinds = kinds
        self._images = None

        torch = self._open(device, 'SeriesSummarizer')
        dev, n = self.device, self.shape[0] * self.shape[1]
        self._chain = 'mean16' in kinds or 'max16' in kinds
        self._xy = 'corr' in kinds
        # state: written by the chunk with t0 == 0, so never cleared here
        self.sum = torch.empty(n, dtype=torch.int64, device=dev)
        self.sumsq = torch.empty(n, dtype=torch.int64, device=dev)
        self.vmax = torch.empty(n, dtype=torch.int32, device=dev)
        self.mean16 = torch.empty(n, dtype=torch.int16, device=dev) if self._chain else None      # float16 BITS
        self.max16 = torch.empty(n, dtype=torch.int16, device=dev) if self._chain else None
        self.xy = torch.empty((4, n), dtype=torch.int64, device=dev) if self._xy else None
        if self._seg is not None:        # the pooled numerators: 16-byte {lo, hi} words, added to by every fold
            self._pvar = torch.zeros((n, 2), dtype=torch.int64, device=dev)
            self._pcov = torch.zeros((4, n, 2), dtype=torch.int64, device=dev) if self._xy else None
            self._sum_total = torch.zeros(n, dtype=torch.int64, device=dev)
            self._vmax_total = torch.full((n,), -2 ** 31, dtype=torch.int32, device=dev)
        self._constructed()

    def _chunk(self, fp, tc, t0, st):
        H, W = self.shape
        self._images = None
        if self._seg is None:
            return self._accumulate(fp, tc, t0, self.n_frames, st)
        # a chunk is cut at the segment boundaries: the part before one is accumulated from its own frame pointer with t0
        # counted from the segment's start (0 initialises the state), then the segment is folded
        for k, m, within, ends in self._seg.cut(t0, tc):
            self._accumulate(fp + k * H * W * 2, m, within, within + m, st)
            if ends is not None:
                self.L.dc_series_fold_segment(self.sum.data_ptr(), self.sumsq.data_ptr(), self.xy.data_ptr() if self._xy else None,
                                              self.vmax.data_ptr(), ends[1], ends[2], self._pvar.data_ptr(),
                                              self._pcov.data_ptr() if self._xy else None, self._sum_total.data_ptr(),
                                              self._vmax_total.data_ptr(), H, W, st)

    def _accumulate(self, fp, tc, t0, n_total, st):
        H, W = self.shape
        self.L.dc_series_accumulate(fp, self._unsigned, tc, t0, n_total,
                                    self.mean16.data_ptr() if self._chain else None,
                                    self.max16.data_ptr() if self._chain else None,
                                    self.sum.data_ptr(), self.sumsq.data_ptr(), self.vmax.data_ptr(), H, W, st)
        if self._xy:
            self.L.dc_series_accumulate_xy(fp, self._unsigned, tc, t0, self.xy.data_ptr(), H, W, st)

    def _finalize(self):
        if self._images is None:
            torch, L = self._torch, self.L
            H, W = self.shape
            with torch.cuda.device(self.device):
                out = torch.empty((3, H * W), dtype=torch.float32, device=self.device)
                if self._seg is not None:
                    L.dc_series_finalize_pooled(self._pvar.data_ptr(), self._pcov.data_ptr() if self._xy else None,
                                                self._sum_total.data_ptr(), out[0].data_ptr(), out[1].data_ptr(),
                                                out[2].data_ptr() if self._xy else None, H, W, self._seg.M, self.n_frames,
                                                self._stream().cuda_stream)
                    self._images = out
                    return out
                L.dc_series_finalize(self.sum.data_ptr(), self.sumsq.data_ptr(), self.xy.data_ptr() if self._xy else None,
                                     out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr() if self._xy else None,
                                     H, W, self.n_frames, self._stream().cuda_stream)
            self._images = out
        return self._images

    def _pooled_moments(self):
        """Detrend mode: the pooled numerators as exact Python ints -- dict(M, T, var (H,W) object array of N(x,x), cov (4,H,W) of
        N(x, neighbour) for right, down, down-right, down-left (None without 'corr'; 0 where the neighbour is outside))."""
        H, W = self.shape
        var = _pooled_ints(self._pvar.cpu().numpy()).reshape(H, W)
        cov = _pooled_ints(self._pcov.cpu().numpy()).reshape(4, H, W) if self._xy else None
        return dict(M=self._seg.M, T=self.n_frames, var=var, cov=cov)

    def _standardize(self, img):
        torch, L = self._torch, self.L
        H, W = self.shape
        with torch.cuda.device(self.device):
            ws = torch.empty(int(L.dc_series_standardize_ws_floats(H, W)) // 2, dtype=torch.float64, device=self.device)
            L.dc_image_standardize(img.data_ptr(), img.data_ptr(), ws.data_ptr(), H, W, self._stream().cuda_stream)
        return img

    def result(self, kind, standardize=False):
        """The (H,W) summary: float32 (float16 for 'mean16', int16 for 'max16').  standardize=True: (img - mean) / std of the
        float32 image, as _summarize_series does with series/mean -- always float32.  With detrend_frames, 'moments' gives the
        pooled numerators as exact Python ints: dict(M, T, var (H,W), cov (4,H,W) or None)."""
        if kind == 'moments' and self._seg is not None:
            if self.fed != self.n_frames:
                raise ValueError('result() after %d of %d frames' % (self.fed, self.n_frames))
            return self._pooled_moments()
        _check_kind(kind, self.kinds)
        if self.fed != self.n_frames:
            raise ValueError('result() after %d of %d frames' % (self.fed, self.n_frames))
        torch = self._torch
        H, W = self.shape
        if kind == 'max' and self._seg is not None:
            raw = self._vmax_total.cpu().numpy().astype(np.float32).reshape(H, W)
        elif kind == 'mean16':
            raw = self.mean16.cpu().numpy().view(np.float16).reshape(H, W)
        elif kind == 'max16':
            raw = self.max16.cpu().numpy().reshape(H, W)
        elif kind == 'max':
            raw = self.vmax.cpu().numpy().astype(np.float32).reshape(H, W)
        else:
            img = self._finalize()[('mean', 'std', 'corr').index(kind)]
            if standardize:
                return self._standardize(img.clone()).cpu().numpy().reshape(H, W)
            return img.cpu().numpy().reshape(H, W)
        if not standardize:
            return raw
        with np.errstate(over='ignore'):
            img = torch.from_numpy(np.ascontiguousarray(raw.astype(np.float32)).reshape(-1)).to(self.device)
        return self._standardize(img).cpu().numpy().reshape(H, W)


MAX_BIN_FRAMES = 64                   # DC_SERIES_MAX_BIN_FRAMES: the frames of one temporal bin


def _check_bin_frames(bin_frames, n_frames=None):
    """The `bin_frames=` keyword: an integer in [1, MAX_BIN_FRAMES], and no more than the recording holds.  Host only."""
    if isinstance(bin_frames, bool) or not isinstance(bin_frames, (int, np.integer)):
        raise ValueError('bin_frames must be an integer in [1, %d], not %r' % (MAX_BIN_FRAMES, bin_frames))
    b = int(bin_frames)
    if not 1 <= b <= MAX_BIN_FRAMES:
        raise ValueError('bin_frames must be in [1, %d], not %d' % (MAX_BIN_FRAMES, b))
    if n_frames is not None and n_frames < b:
        raise ValueError('bin_frames = %d, the recording has only %d frames' % (b, n_frames))
    return b


class TemporalBinner(_FrameReader):
    """Temporal binning in front of the readers: the recording's frames in, the means of `bin_frames` consecutive frames out, on
    the device (dc_series_bin_time).  A bin's value is floor((2 s + b) / (2 b)) of the exact sum s of its b frames -- the mean
    rounded half up, the rule of make_template and dc_motion_bin -- in the recording's own 16-bit type, so every reader takes the
    binned frames as it takes the raw ones.  The trailing n_frames % bin_frames frames close no bin and are dropped, as
    dc_motion_bin drops trailing rows.  Chunk boundaries never change a bit.

        tb = TemporalBinner((H, W), T, np.int16, bin_frames=4)
        reader = RoiPairCorr((H, W), tb.n_out, np.int16, rois)
        for chunk in chunks:
            binned = tb.feed(chunk)
            if binned.shape[0]: reader.feed(binned)

    n_out = n_frames // bin_frames; fed: frames consumed so far; emitted: bins written so far."""
    _stage_tag, _noun = 'tbin_stage', 'binner'

    def __init__(self, shape, n_frames, dtype, bin_frames=4, shifts=None, fine_shifts=None, bidi=0, device=None, chunk_frames=None):
        """shifts / fine_shifts / bidi: as for SeriesSummarizer, applied BEFORE the sum (dc_bidi_apply, then the shift move, fill
        0): the means are means of registered frames.  bin_frames: an integer in [1, 64], at most n_frames; 1 is a copy."""
        # ---- everything that can be wrong with the arguments is a ValueError before the library or the GPU is touched ----
        self._declare(shape, n_frames, dtype, chunk_frames, shifts, fine_shifts, bidi)
        self.bin_frames = _check_bin_frames(bin_frames, self.n_frames)
        self.n_out = self.n_frames // self.bin_frames
        self.emitted = 0

        torch = self._open(device, 'TemporalBinner')
        # the open bin's sum: read only once a call has left frames in it, so never cleared here
        self._carry = torch.empty(self.shape[0] * self.shape[1], dtype=torch.int32, device=self.device)
        self._constructed()

    def feed(self, frames):
        """The next frames of the recording, any t >= 1: what SeriesSummarizer.feed takes (numpy or memmap chunks of the
        recording's dtype, staged through two pinned slots; or a contiguous (t, H, W) torch.int16 tensor on the binner's device,
        read in place).  -> the bins this feed closed: a contiguous (k, H, W) torch.int16 tensor on the device holding the bits of
        the recording's dtype, k >= 0.  It is a FRESH allocation every time, written on the current stream: no later feed touches
        it, and a reader fed on the same stream right away reads it after the kernels that wrote it."""
        return super(TemporalBinner, self).feed(frames)

    def _begin_feed(self, t):
        out = self._torch.empty(((self.fed % self.bin_frames + t) // self.bin_frames,) + self.shape, dtype=self._torch.int16, device=self.device)
        self._dst = out.data_ptr()           # where the next bin goes
        return out, True

    def _chunk(self, fp, tc, t0, st):
        (H, W), b = self.shape, self.bin_frames
        k = (t0 % b + tc) // b
        self.L.dc_series_bin_time(fp, self._unsigned, tc, H, W, b, t0 % b, self._carry.data_ptr(), self._dst if k else None, st)
        self._dst += 2 * H * W * k
        self.emitted += k


def _open_series(dspath, source):
    """(frames array-like of (T,H,W), close()) without reading the recording: .npz members and contiguous HDF5 datasets are
    memory-mapped, h5py datasets are sliced chunk by chunk."""
    key = source.replace('/', '_', 1)
    if str(dspath).endswith('.npz'):
        import zipfile
        with zipfile.ZipFile(dspath) as z:
            names = z.namelist()
            if key + '.npy' not in names:
                raise ValueError('%s has no member %r' % (dspath, key))
            info = z.getinfo(key + '.npy')
            stored = info.compress_type == zipfile.ZIP_STORED
        if stored:                      # np.savez: members are stored, the .npy payload can be mapped in place
            with open(dspath, 'rb') as fp:
                fp.seek(info.header_offset)
                head = fp.read(30)
                nlen, xlen = int.from_bytes(head[26:28], 'little'), int.from_bytes(head[28:30], 'little')
                fp.seek(info.header_offset + 30 + nlen + xlen)
                version = np.lib.format.read_magic(fp)
                shape, fortran, dt = (np.lib.format.read_array_header_1_0(fp) if version == (1, 0)
                                      else np.lib.format.read_array_header_2_0(fp))
                offset = fp.tell()
            if not fortran and not dt.hasobject:
                return np.memmap(dspath, dtype=dt, mode='r', offset=offset, shape=shape), (lambda: None)
        z = np.load(dspath, allow_pickle=False)      # compressed member: has to be inflated
        return z[key], z.close
    from .unet2ds import _open_dataset            # the h5py / built-in reader choice of the default summary functions
    _, fp = _open_dataset(dspath)

    def close():
        try:
            fp.close()
        except BufferError:            # a slice of the mapping is still alive (a traceback holds it): the collector closes the file
            pass
    try:
        node = fp[source]
    except KeyError:
        close()
        raise ValueError('%s has no dataset %r' % (dspath, source))
    if hasattr(node, 'view'):          # hdf5_min: the dataset in place, no copy
        from . import hdf5_min
        try:
            return node.view(), close
        except hdf5_min.Hdf5Error:     # compact / unallocated storage: small enough to read
            return node.read(), close
    return node, close                 # h5py: sliced chunk by chunk


def _open_recording(dspath, source):
    """_open_series, and the check that what it opened is a (T,H,W) recording (closed again if it is not)."""
    frames, close = _open_series(dspath, source)
    if len(frames.shape) != 3:
        shape, frames = tuple(frames.shape), None
        close()
        raise ValueError('%s of %s is not a (T,H,W) recording: %r' % (source, dspath, shape))
    return frames, close


def summarize_series_device(dspath, kind='mean', standardize=True, source='series/raw', device=None, chunk_frames=None,
                            shifts=None, fine_shifts=None, bin_frames=None, detrend_frames=None, keep=None, bidi=0):
    """Drop-in `series_summary_func`: streams `source` of the dataset through a SeriesSummarizer and returns the (H,W)
    float32 summary (standardised like _summarize_series's by default).  shifts: the (T, 2) (dy, dx) of every frame, or
    its (T, By, Bx, 2) block shifts (motion.estimate_shifts_device), applied on the device on the way in.  fine_shifts: instead,
    either shape in sixteenths of a pixel (estimate_shifts_device(subpixel=True)): the frames are interpolated on the way in.
    bidi: the offset of the odd lines (motion.estimate_bidi_device), undone on the way in before the shifts.
    bin_frames: None, or an integer b in [1, 64]: the corrected frames pass through a TemporalBinner first and the summary is that
    of the T // b rounded means of b consecutive frames (the trailing T % b frames are dropped; 1 gives what None gives).  `std`
    and `corr` of a binned recording are not comparable with the unbinned ones.
    detrend_frames: None, or an integer L in [2, 4096]: `std` and `corr` pooled over segments of L frames (SeriesSummarizer); with
    bin_frames, L counts binned frames.  Results at different L are not comparable with each other or with None.
    keep: None, or a (T,) array of booleans (frames.flag_frames): the frames marked False are left out by a frames.FrameFilter after
    bidi and the shifts and before binning and detrending, whose b and L then count kept frames; all True gives what None gives."""
    _check_kind(kind)
    if detrend_frames is not None:
        _check_detrend_frames(detrend_frames)
        if kind in ('mean16', 'max16'):
            raise ValueError('mean16 / max16 are the stored summaries of the whole recording: not served with detrend_frames')

    def reader_of(shape, n_frames, dtype, **kw):
        return SeriesSummarizer(shape, n_frames, dtype, kinds=(kind,), detrend_frames=detrend_frames, **kw)
    summ = _read_recording(dspath, source, reader_of, device, chunk_frames, shifts, fine_shifts, bidi, bin_frames, keep)
    out = summ.result(kind, standardize=standardize)
    return np.asarray(out, dtype=np.float32)
