"""Motion correction on the device, rigid or piecewise-rigid: the frames of a recording (T,H,W) of 16-bit frames are registered
to a template.

Every other stage of the pipeline (series.py, UNet2DSummary.predict, traces.py, spikes.py) assumes registered frames.  Here every
frame is compared with a template at every whole-pixel shift within +-max_shift (dc_motion_ssd: the exact integer sum of
squared differences over the template's interior), the best shift is picked (dc_motion_pick) and the frame is moved
(dc_motion_apply) -- include/dcunet.h:

    what          dtype            exactness
    scores        int64            exact: (t, 2S+1, 2S+1) sums of squared differences, dy the slow axis, index dy + S
    shifts        int32 (t, 2)     exact: argmin of (score, dy^2 + dx^2, dy, dx) -- ties go to the smallest displacement
    corrected     the frames'      exact: out[y, x] = frame[y + dy, x + dx], `fill` outside the frame

Sign convention: a shift (dy, dx) means out[y, x] = frame[y + dy, x + dx]; a frame cut from a scene at offset (+a, +b) relative
to the template is found as (dy, dx) = (-a, -b).

    mc = MotionCorrector((H, W), T, np.int16, template, max_shift=8)
    for chunk in chunks: corrected = mc.feed(chunk)        # an int16 CUDA tensor: SeriesSummarizer / RoiTraceExtractor take it
    shifts, rect = mc.shifts(), mc.valid()

    shifts, template = estimate_shifts_device('dataset.hdf5')                 # one pass over the recording
    img = summarize_series_device('dataset.hdf5', kind='corr', shifts=shifts)  # corrected on the way in, no second copy
    traces = extract_traces_device('dataset.hdf5', mask, shifts=shifts)

Piecewise-rigid (blocks=(By, Bx)): a frame is scanned line by line while the tissue moves, so one translation cannot register
all of it.  The frame is cut into By x Bx blocks (block i covers rows [floor(i H / By), floor((i+1) H / By)), columns likewise);
every block gets the frame's rigid shift plus a residual within +-max_dev, found the same way over the block's own pixels
(dc_motion_block_ssd, dc_motion_block_pick: ties go to the smallest residual, so a featureless block follows the rigid shift),
and the block shifts are blended bilinearly between the block centres into one whole-pixel shift per pixel (dc_motion_warp).
Where that field changes by one pixel a source pixel is repeated or skipped: the price of whole-pixel exactness.

    mc = MotionCorrector((H, W), T, np.int16, template, max_shift=8, blocks=(4, 4), max_dev=3)
    for chunk in chunks: corrected = mc.feed(chunk)        # warped by the field
    bs = mc.block_shifts()                                 # (fed, By, Bx, 2) int32; mc.shifts() stays the rigid table

    bs, template = estimate_shifts_device('dataset.hdf5', blocks=(4, 4))      # (T, By, Bx, 2): shifts= takes it as it is

Sub-pixel (subpixel=True): every pick -- the frame's, and with blocks every block's -- is refined to a sixteenth of a pixel from
the scores next to it (dc_motion_refine, dc_motion_block_refine: the vertex of the parabola through the picked score and its two
neighbours, per axis), and the frames are interpolated bilinearly at the fine shift or the fine shift field (dc_motion_apply_sub,
dc_motion_warp_sub).  Still integers only -- fine shifts are int32 in sixteenths, the interpolation weights are sixteenths:

    what          dtype            exactness
    fine shifts   int32 (t, 2)     exact: 16 * pick + q, q = sign(N) floor((16 |N| + D - 1) / (2 D)) in [-8, 8] per axis,
                  (t, By, Bx, 2)   N = s(-1) - s(+1), D = s(-1) - 2 s(0) + s(+1); 0 at the table's border and where D = 0
    corrected     the frames'      exact: floor(((16-fy) ((16-fx) a00 + fx a01) + fy ((16-fx) a10 + fx a11) + 128) / 256) with
                                   (iy, fy) = divmod(sy, 16), a_ij = frame[y + iy + i, x + ix + j]; `fill` where a tap that
                                   is used (weight > 0) lies outside the frame

    mc = MotionCorrector((H, W), T, np.int16, template, max_shift=8, subpixel=True)
    for chunk in chunks: corrected = mc.feed(chunk)        # interpolated
    fine = mc.fine_shifts()                                # (fed, 2) int32 sixteenths; fine_to_pixels(fine) = fine / 16
    fine, template = estimate_shifts_device('dataset.hdf5', subpixel=True)
    img = summarize_series_device('dataset.hdf5', kind='corr', fine_shifts=fine)

Interpolation averages up to four values, so at fractional shifts it lowers the pixel noise: `std` and `corr` of a
sub-pixel-corrected recording are not comparable bit for bit with those of a whole-pixel-corrected one.

Wide search (coarse=c, c in 2, 4, 8; max_shift in [c, 16 c], so up to 128): the exhaustive search costs (2S+1)^2 passes and is
capped at 16 pixels, less than a behaving animal moves the field of view.  With coarse=c frames and template are binned c x c
(dc_motion_bin: the mean rounded half up, trailing rows and columns dropped), the unchanged exhaustive search finds a coarse
shift on the binned frames within +-ceil(max_shift / c), and the full-resolution scores are computed only within +-c of c times
that shift, clamped so that the window stays inside +-max_shift (dc_motion_ssd_around, dc_motion_pick_around):

    what            dtype            exactness
    coarse shifts   int32 (t, 2)     exact: the pick of the binned frames against the binned template, unscaled
    scores          int64            exact: (t, 2c+1, 2c+1), the entries centre + (ey, ex) of the exhaustive table of radius S,
                                     centre = clamp(c * coarse, -(S - c), S - c) per component
    shifts          int32 (t, 2)     exact: the argmin of (score, dy^2 + dx^2, dy, dx) over the TOTAL shifts of the window

This is NOT the exhaustive argmin of radius max_shift: it is that argmin whenever it lies within +-c of the clamped c * coarse
pick (a scene whose coarse structure is ambiguous can send the window to the wrong place).  With subpixel=True the pick is
refined within the window table; a pick on the window's border is not refined (q = 0 on that axis).

    mc = MotionCorrector((H, W), T, np.int16, template, max_shift=48, coarse=4)
    for chunk in chunks: corrected = mc.feed(chunk)
    shifts, coarse = mc.shifts(), mc.coarse_shifts()
    shifts, template = estimate_shifts_device('dataset.hdf5', max_shift=48, coarse=4)

Bidirectional scan-phase correction (bidi=p): a resonant scanner draws even lines left to right and odd lines right to left, and a
phase error between the sweeps displaces all odd lines horizontally by a constant few pixels.  That offset is found once per
recording by an exhaustive search within +-max_offset (dc_bidi_scores, summed over frames, picked on the host) and undone as a
pure move of the odd lines (dc_bidi_apply) BEFORE anything else reads a frame -- the template is built from corrected lines:

    what          dtype            exactness
    scores        int64            exact: (t, 2P+1), index p + P: the sum over odd y in [1, H-1), x in [P, W-P) of
                                   (2 f[y, x+p] - f[y-1, x] - f[y+1, x])^2
    totals        Python ints      exact: the scores summed over the frames fed (a sum over frames need not fit 64 bits)
    offset        int              exact: argmin of (total, p^2, p) -- 0 wins every tie it is part of
    corrected     the frames'      exact: out[y, x] = frame[y, x + p] for odd y (`fill` outside the row), even rows copied

Sign convention: odd lines recorded as frame[y, x] = scene[y, x + b] are found as p = -b.

    est = BidiEstimator((H, W), np.int16, max_offset=8)
    for chunk in chunks: est.feed(chunk)
    p = est.offset()
    p, totals = estimate_bidi_device('dataset.hdf5')                          # the first 200 frames
    mc = MotionCorrector((H, W), T, np.int16, template, max_shift=8, bidi=p)   # feed() returns frames with both corrections
    shifts, template = estimate_shifts_device('dataset.hdf5', bidi=p)
    img = summarize_series_device('dataset.hdf5', kind='corr', shifts=shifts, bidi=p)

With sub-pixel shifts the columns outside valid_rectangle(..., bidi=p) hold blends of `fill`, as they already do at the frame's edge.
The move leaves |p| columns of `fill` at one edge of the odd lines, which the shift search counts as a mismatch at every shift that
reaches them: choose max_shift at least the largest expected shift plus |p|.
Whole-pixel offsets, one per recording, odd lines only: a sub-pixel or per-frame offset is not built.

Scope: shifts found by exhaustive whole-pixel search, max_shift <= 16 -- or by the two-level wide search, max_shift <= 128,
rigid only --, max_dev <= 8, at most 32 x 32 blocks, refined to 1/16 pixel by a parabola fit, bilinear interpolation.  Template
building with sub-pixel or block shifts, temporal smoothing of the shifts, FFT methods, other interpolation kernels,
piecewise-rigid blocks on top of a wide search and more than two levels are not implemented.

Importing this module needs neither torch nor the GPU; constructing a MotionCorrector does (there is no CPU fallback).
"""
import numpy as np

from ._reader import _CHUNK_BYTES, _FrameReader, _check_bidi, _check_shape, _frame_dtype, _open_device
from .series import MAX_BIDI, _open_recording

MAX_SHIFT = 16                        # DC_MOTION_MAX_SHIFT
MAX_DEV = 8                           # DC_MOTION_MAX_DEV
MAX_BLOCKS = 32                       # DC_MOTION_MAX_BLOCKS
SUBPIXEL = 16                         # DC_MOTION_SUB: fine shifts are int32 in units of 1 / SUBPIXEL of a pixel
MAX_WIDE_SHIFT = 128                  # DC_MOTION_MAX_WIDE_SHIFT: the largest max_shift of the wide search (coarse=8)
COARSE = (2, 4, 8)                    # the binning factors of the wide search


def _check_max_shift(max_shift, shape=None):
    if isinstance(max_shift, bool) or not isinstance(max_shift, (int, np.integer)):
        raise ValueError('max_shift must be an integer in [0, %d], not %r' % (MAX_SHIFT, max_shift))
    S = int(max_shift)
    if not 0 <= S <= MAX_SHIFT:
        raise ValueError('max_shift must be in [0, %d], not %d' % (MAX_SHIFT, S))
    if shape is not None and (shape[0] <= 2 * S or shape[1] <= 2 * S):
        raise ValueError('max_shift = %d leaves no interior in a %d x %d frame: H > 2 * max_shift and W > 2 * max_shift'
                         % (S, shape[0], shape[1]))
    return S


def _check_coarse(coarse, max_shift, shape=None, blocks=None):
    """coarse=c and max_shift of the wide search -> (c, S): c in 2, 4, 8, S in [c, 16 c], and the frame keeps an interior at both
    levels: H > 2S, W > 2S, and floor(H / c) > 2 ceil(S / c), floor(W / c) > 2 ceil(S / c) for the binned frame."""
    if isinstance(coarse, bool) or not isinstance(coarse, (int, np.integer)) or int(coarse) not in COARSE:
        raise ValueError('coarse must be None or one of 2, 4, 8, not %r' % (coarse,))
    c = int(coarse)
    if blocks is not None:
        raise ValueError('blocks together with coarse = %d is not built: the piecewise-rigid mode needs max_shift <= %d' % (c, MAX_SHIFT))
    if isinstance(max_shift, bool) or not isinstance(max_shift, (int, np.integer)):
        raise ValueError('max_shift must be an integer in [%d, %d] with coarse = %d, not %r' % (c, MAX_SHIFT * c, c, max_shift))
    S = int(max_shift)
    if not c <= S <= MAX_SHIFT * c:
        raise ValueError('max_shift must be in [%d, %d] with coarse = %d, not %d' % (c, MAX_SHIFT * c, c, S))
    if shape is not None:
        H, W = shape
        Sc = -(-S // c)
        if H <= 2 * S or W <= 2 * S:
            raise ValueError('max_shift = %d with coarse = %d leaves no interior in a %d x %d frame: H > 2 * max_shift and '
                             'W > 2 * max_shift' % (S, c, H, W))
        if H // c <= 2 * Sc or W // c <= 2 * Sc:
            raise ValueError('coarse = %d leaves no interior in the binned %d x %d frame at the coarse radius %d'
                             % (c, H // c, W // c, Sc))
    return c, S


def _check_bidi_radius(max_offset, shape=None):
    """max_offset of the scan-phase search -> P in [0, MAX_BIDI]; the frame must keep an odd line between two even ones and an
    interior column: H >= 3 and W > 2P."""
    if isinstance(max_offset, bool) or not isinstance(max_offset, (int, np.integer)):
        raise ValueError('max_offset must be an integer in [0, %d], not %r' % (MAX_BIDI, max_offset))
    P = int(max_offset)
    if not 0 <= P <= MAX_BIDI:
        raise ValueError('max_offset must be in [0, %d], not %d' % (MAX_BIDI, P))
    if shape is not None:
        if shape[0] < 3:
            raise ValueError('a %d x %d frame has no odd line between two even ones: H >= 3' % (shape[0], shape[1]))
        if shape[1] <= 2 * P:
            raise ValueError('max_offset = %d leaves no interior column in a %d x %d frame: W > 2 * max_offset' % (P, shape[0], shape[1]))
    return P


def pick_bidi(totals):
    """The offset of the 2P+1 totals (index p + P; any integers, Python ints beyond 64 bits included): the p that minimises
    (total, p^2, p) -- 0 wins every tie it is part of, then the smaller |p|, then the negative one.  Host only."""
    totals = [int(v) for v in totals]
    if len(totals) < 1 or len(totals) % 2 != 1:
        raise ValueError('totals must hold 2P+1 values, not %d' % len(totals))
    P = len(totals) // 2
    return min(range(-P, P + 1), key=lambda p: (totals[p + P], p * p, p))


def block_edges(n, B):
    """The B + 1 edges of the blocks of an axis of n pixels: e(i) = floor(i * n / B)."""
    return [i * n // B for i in range(B + 1)]


def _check_blocks(blocks, max_dev, shape=None, max_shift=0):
    """blocks=(By, Bx) and max_dev of the piecewise-rigid mode -> (By, Bx, D); every block, clipped to the interior that
    max_shift + max_dev leaves, must keep a pixel."""
    try:
        ok = len(blocks) == 2 and all(isinstance(b, (int, np.integer)) and not isinstance(b, bool) for b in blocks)
    except TypeError:
        ok = False
    if not ok:
        raise ValueError('blocks must be (By, Bx), two integers in [1, %d], not %r' % (MAX_BLOCKS, blocks))
    By, Bx = int(blocks[0]), int(blocks[1])
    if not (1 <= By <= MAX_BLOCKS and 1 <= Bx <= MAX_BLOCKS):
        raise ValueError('blocks must be (By, Bx), two integers in [1, %d], not %r' % (MAX_BLOCKS, (By, Bx)))
    if isinstance(max_dev, bool) or not isinstance(max_dev, (int, np.integer)):
        raise ValueError('max_dev must be an integer in [0, %d], not %r' % (MAX_DEV, max_dev))
    D = int(max_dev)
    if not 0 <= D <= MAX_DEV:
        raise ValueError('max_dev must be in [0, %d], not %d' % (MAX_DEV, D))
    if shape is not None:
        M = int(max_shift) + D
        for n, B, axis in ((shape[0], By, 'rows'), (shape[1], Bx, 'columns')):
            e = block_edges(n, B)
            if n < B or n <= 2 * M or min(e[1], n - M) <= M or max(e[B - 1], M) >= n - M:
                raise ValueError('blocks = %r: a block of a %d x %d frame has no %s inside the margin max_shift + max_dev = %d'
                                 % ((By, Bx), shape[0], shape[1], axis, M))
    return By, Bx, D


def _check_subpixel(subpixel):
    if not isinstance(subpixel, (bool, np.bool_)):
        raise ValueError('subpixel must be True or False, not %r' % (subpixel,))
    return bool(subpixel)


def _check_fill(fill):
    if isinstance(fill, bool) or not isinstance(fill, (int, np.integer)) or not -32768 <= int(fill) <= 65535:
        raise ValueError('fill must be a 16-bit integer value, not %r' % (fill,))
    return int(fill)


def _check_template(template, shape, dtype):
    if not isinstance(template, np.ndarray):
        raise ValueError('template must be a numpy array, not %s' % type(template).__name__)
    if tuple(template.shape) != tuple(shape):
        raise ValueError('template is %r, the frames are %r' % (tuple(template.shape), tuple(shape)))
    if template.dtype != dtype:
        raise ValueError('template is %s, the recording was declared %s' % (template.dtype, dtype))
    return np.ascontiguousarray(template)


def valid_rectangle(shifts, shape, fine=False, bidi=0):
    """((y0, y1), (x0, x1)): the rectangle every frame corrected by `shifts` (n, 2) covers with its own pixels,
    y in [max(0, -min dy), H - max(0, max dy)), likewise x.  Block shifts (n, By, Bx, 2) are taken one by one: the shift field
    never leaves their range, so the rectangle bounds the warped frames too.  fine=True: `shifts` are fine shifts (sixteenths of a
    pixel) and an interpolated pixel needs every tap it uses: y0 = max(0, -floor(min sy / 16)), y1 = H - max(0, ceil(max sy / 16)),
    likewise x.  bidi=p: the odd lines were moved by p first (dc_bidi_apply), and an odd line is valid only where both moves stay
    inside: the column limits are taken over the union of the x shifts and the x shifts plus p (plus 16 p with fine), by the same
    formulas; shifts=None: no registration, the columns are [max(0, -p), W - max(0, p)).  With sub-pixel shifts the columns
    outside this rectangle hold blends of `fill`, as they already do at the frame's edge.  Host only."""
    H, W = shape
    if not isinstance(fine, (bool, np.bool_)):
        raise ValueError('fine must be True or False, not %r' % (fine,))
    p = _check_bidi(bidi, shape)
    if shifts is None:
        return (0, H), (max(0, -p), W - max(0, p))
    s = np.asarray(shifts).reshape(-1, 2).astype(np.int64)
    if len(s) == 0:
        return (0, H), (max(0, -p), W - max(0, p))
    lo, hi = s.min(axis=0), s.max(axis=0)
    if p:
        k = p * SUBPIXEL if fine else p
        lo[1], hi[1] = min(lo[1], lo[1] + k), max(hi[1], hi[1] + k)
    if fine:
        lo, hi = lo // SUBPIXEL, -((-hi) // SUBPIXEL)        # floor and ceiling for either sign
    return ((max(0, -int(lo[0])), H - max(0, int(hi[0]))), (max(0, -int(lo[1])), W - max(0, int(hi[1]))))


def fine_to_pixels(fine):
    """Fine shifts (integers in sixteenths of a pixel, any shape) as float64 pixels: fine / 16, exact.  Host only."""
    a = np.asarray(fine)
    if a.dtype.kind not in 'iu':
        raise ValueError('fine shifts are integers (sixteenths of a pixel), not %s' % a.dtype)
    return a.astype(np.float64) / SUBPIXEL


class MotionCorrector(_FrameReader):
    """Owns the device state of one recording's registration; feed() the frames in order, in chunks of any size."""
    _stage_tag, _noun = 'motion_stage', 'corrector'

    def __init__(self, shape, n_frames, dtype, template, max_shift=8, fill=0, device=None, chunk_frames=None, blocks=None,
                 max_dev=3, subpixel=False, coarse=None, bidi=0):
        # ---- everything that can be wrong with the arguments is a ValueError before the library or the GPU is touched ----
        self._declare(shape, n_frames, dtype, chunk_frames, max_frames=None)
        shape, n_frames = self.shape, self.n_frames
        H, W = shape
        self.coarse = None
        if coarse is None:
            self.max_shift = _check_max_shift(max_shift, shape)
        else:                              # the wide search: max_shift in [c, 16 c], rigid only
            self.coarse, self.max_shift = _check_coarse(coarse, max_shift, shape, blocks)
        self.fill = _check_fill(fill)
        self.subpixel = _check_subpixel(subpixel)
        self.blocks, self.max_dev = None, None
        if blocks is not None:
            By, Bx, self.max_dev = _check_blocks(blocks, max_dev, shape, self.max_shift)
            self.blocks = (By, Bx)
        self.bidi = _check_bidi(bidi, shape)         # its own move, with its own fill: not the base's corrections
        template = _check_template(template, shape, self.dtype)
        self._last = 0

        torch = self._open(device, 'MotionCorrector')
        dev, nd = self.device, 2 * (self.max_shift if self.coarse is None else self.coarse) + 1
        self.template = template
        self._tmpl = torch.from_numpy(template.view(np.int16)).to(dev)
        self._shifts = torch.zeros((n_frames, 2), dtype=torch.int32, device=dev)
        self._scores = torch.empty((self.chunk_frames, nd, nd), dtype=torch.int64, device=dev)      # fully written by every chunk
        if self.coarse is not None:        # the binned template, made once; the chunk's binned frames and their coarse tables
            c = self.coarse
            Hc, Wc, Sc = H // c, W // c, -(-self.max_shift // c)
            self._cshape, self._cradius = (Hc, Wc), Sc
            self._tmpl_c = torch.empty((Hc, Wc), dtype=torch.int16, device=dev)
            self._binned = torch.empty((self.chunk_frames, Hc, Wc), dtype=torch.int16, device=dev)
            self._cscores = torch.empty((self.chunk_frames, 2 * Sc + 1, 2 * Sc + 1), dtype=torch.int64, device=dev)
            self._coarse = torch.zeros((n_frames, 2), dtype=torch.int32, device=dev)
            with torch.cuda.device(dev):
                self.L.dc_motion_bin(self._tmpl.data_ptr(), self._unsigned, 1, H, W, c, self._tmpl_c.data_ptr(),
                                     self._stream().cuda_stream)
        if self.blocks is not None:
            (By, Bx), nb = self.blocks, 2 * self.max_dev + 1
            self._bshifts = torch.zeros((n_frames, By, Bx, 2), dtype=torch.int32, device=dev)
            self._bscores = torch.empty((self.chunk_frames, By, Bx, nb, nb), dtype=torch.int64, device=dev)
        if self.subpixel:                  # the fine shifts (sixteenths) beside the whole-pixel picks they refine
            self._fine = torch.zeros((n_frames, 2) if self.blocks is None else (n_frames,) + self.blocks + (2,), dtype=torch.int32, device=dev)
        if self.bidi:                      # one chunk of frames whose odd lines have been moved: what everything below reads
            self._bidi_scratch = torch.empty((self.chunk_frames, H, W), dtype=torch.int16, device=dev)
        self._constructed()                # feed() may run on another stream: it waits for the fills and the binned template

    def _register(self, fp, tc, t0, out, st):
        """The launches of one piece of at most chunk_frames frames at fp, frames [t0, t0 + tc); out: where the corrected frames
        go, or None."""
        H, W = self.shape
        L, S = self.L, self.max_shift
        uns = self._unsigned
        rows = self._shifts.data_ptr() + 8 * t0
        if self.bidi:                      # the scan-phase offset first: scores, picks and movers read the corrected lines
            L.dc_bidi_apply(fp, tc, self.bidi, H, W, self.fill, self._bidi_scratch.data_ptr(), st)
            fp = self._bidi_scratch.data_ptr()
        if self.coarse is not None:
            # the wide search: the exhaustive pick on the binned frames, then the full-resolution window around c times it
            c, (Hc, Wc), Sc = self.coarse, self._cshape, self._cradius
            crows = self._coarse.data_ptr() + 8 * t0
            frows = self._fine.data_ptr() + 8 * t0 if self.subpixel else None
            L.dc_motion_bin(fp, uns, tc, H, W, c, self._binned.data_ptr(), st)
            L.dc_motion_ssd(self._binned.data_ptr(), uns, tc, self._tmpl_c.data_ptr(), Hc, Wc, Sc, self._cscores.data_ptr(), st)
            L.dc_motion_pick(self._cscores.data_ptr(), tc, Sc, crows, None, st)
            L.dc_motion_ssd_around(fp, uns, tc, self._tmpl.data_ptr(), H, W, S, c, crows, c, self._scores.data_ptr(), st)
            L.dc_motion_pick_around(self._scores.data_ptr(), crows, c, tc, S, c, rows, None, frows, st)
        else:
            L.dc_motion_ssd(fp, uns, tc, self._tmpl.data_ptr(), H, W, S, self._scores.data_ptr(), st)
            L.dc_motion_pick(self._scores.data_ptr(), tc, S, rows, None, st)
        if self.blocks is not None:
            (By, Bx), D = self.blocks, self.max_dev
            brows = self._bshifts.data_ptr() + 8 * By * Bx * t0
            L.dc_motion_block_ssd(fp, uns, tc, self._tmpl.data_ptr(), H, W, S, D, By, Bx, rows, self._bscores.data_ptr(), st)
            L.dc_motion_block_pick(self._bscores.data_ptr(), rows, tc, By, Bx, S, D, brows, None, st)
            if self.subpixel:
                frows = self._fine.data_ptr() + 8 * By * Bx * t0
                L.dc_motion_block_refine(self._bscores.data_ptr(), rows, brows, tc, By, Bx, S, D, frows, st)
                if out is not None:
                    L.dc_motion_warp_sub(fp, uns, tc, frows, By, Bx, H, W, self.fill, out, st)
            elif out is not None:
                L.dc_motion_warp(fp, tc, brows, By, Bx, H, W, self.fill, out, st)
        elif self.subpixel:
            frows = self._fine.data_ptr() + 8 * t0
            if self.coarse is None:        # the wide search has refined its pick within the window table already
                L.dc_motion_refine(self._scores.data_ptr(), rows, tc, S, frows, st)
            if out is not None:
                L.dc_motion_apply_sub(fp, uns, tc, frows, H, W, self.fill, out, st)
        elif out is not None:
            L.dc_motion_apply(fp, tc, rows, H, W, self.fill, out, st)
        self._last = tc

    def _begin_feed(self, t):
        out = self._torch.empty((t,) + self.shape, dtype=self._torch.int16, device=self.device) if self._correct else None
        self._dst = out.data_ptr() if self._correct else None      # where the next corrected frame goes
        return out, True

    def _chunk(self, fp, tc, t0, st):
        """A resident tensor arrives whole: it is registered in pieces of chunk_frames, the size of the score tables."""
        H, W = self.shape
        for a in range(0, tc, self.chunk_frames):
            n = min(self.chunk_frames, tc - a)
            self._register(fp + 2 * a * H * W, n, t0 + a, self._dst, st)
            if self._dst is not None:
                self._dst += 2 * n * H * W

    def feed(self, frames, correct=True):
        """The next frames of the recording, any t >= 1: a (t, H, W) numpy array or memmap of the recording's dtype (staged
        through two pinned slots), or a contiguous (t, H, W) torch.int16 tensor on the corrector's device holding the
        recording's bits (read in place).  Returns the corrected frames as a (t, H, W) torch.int16 tensor on the device (the
        frames' bits); their shifts land in rows [fed, fed + t) of shifts_device().  correct=False only estimates the shifts
        and returns None.  With blocks: the frames are warped by the shift field, and their block shifts land in rows
        [fed, fed + t) of block_shifts_device().  With subpixel=True every pick is refined to a sixteenth of a pixel (rows
        [fed, fed + t) of fine_shifts_device()) and the frames are interpolated bilinearly at the fine shifts (or the fine
        shift field), `fill` where a tap that is used lies outside the frame.  With bidi=p every piece first has its odd lines
        moved by p (dc_bidi_apply, `fill` where x + p leaves the row): the returned frames carry both corrections."""
        self._correct = correct
        return super(MotionCorrector, self).feed(frames)

    def shifts_device(self):
        """The int32 (n_frames, 2) tensor of (dy, dx) rows on the device; rows [0, fed) are set."""
        return self._shifts

    def shifts(self):
        """(fed, 2) int32 numpy array of the (dy, dx) found so far."""
        return self._shifts[:self.fed].cpu().numpy()

    def last_scores(self):
        """(t, 2S+1, 2S+1) int64 numpy array: the scores of the last piece of at most chunk_frames frames that was registered
        (dy the slow axis, index dy + S) -- score minus the frame's minimum is a confidence measure.  With coarse=c: the window
        table (t, 2c+1, 2c+1) around each frame's centre clamp(c * coarse shift, max_shift - c) (ey the slow axis, index ey + c)."""
        return self._scores[:self._last].cpu().numpy()

    def _need_coarse(self):
        if self.coarse is None:
            raise ValueError('this corrector searches exhaustively: coarse shifts need coarse=2, 4 or 8')

    def coarse_shifts_device(self):
        """The int32 (n_frames, 2) tensor of the coarse picks on the device, in binned pixels (unscaled); rows [0, fed) are set."""
        self._need_coarse()
        return self._coarse

    def coarse_shifts(self):
        """(fed, 2) int32 numpy array: the pick of every binned frame against the binned template, in binned pixels."""
        self._need_coarse()
        return self._coarse[:self.fed].cpu().numpy()

    def last_coarse_scores(self):
        """(t, 2Sc+1, 2Sc+1) int64 numpy array, Sc = ceil(max_shift / coarse): the scores of the binned frames of the last piece
        that was registered."""
        self._need_coarse()
        return self._cscores[:self._last].cpu().numpy()

    def _need_blocks(self):
        if self.blocks is None:
            raise ValueError('this corrector is rigid: block shifts need blocks=(By, Bx)')

    def block_shifts_device(self):
        """The int32 (n_frames, By, Bx, 2) tensor of block shifts on the device; rows [0, fed) are set."""
        self._need_blocks()
        return self._bshifts

    def block_shifts(self):
        """(fed, By, Bx, 2) int32 numpy array: the (dy, dx) of every block, the frame's rigid shift included."""
        self._need_blocks()
        return self._bshifts[:self.fed].cpu().numpy()

    def last_block_scores(self):
        """(t, By, Bx, 2D+1, 2D+1) int64 numpy array: the block scores of the last piece that was registered, around the
        frame's rigid shift (ey the slow axis, index ey + D)."""
        self._need_blocks()
        return self._bscores[:self._last].cpu().numpy()

    def _need_subpixel(self):
        if not self.subpixel:
            raise ValueError('this corrector stops at whole pixels: fine shifts need subpixel=True')

    def fine_shifts_device(self):
        """The int32 (n_frames, 2) tensor of fine shifts (sy, sx) in sixteenths of a pixel on the device -- with blocks the
        (n_frames, By, Bx, 2) fine block shifts --; rows [0, fed) are set.  `fine_shifts=` of SeriesSummarizer /
        RoiTraceExtractor takes it."""
        self._need_subpixel()
        return self._fine

    def fine_shifts(self):
        """(fed, 2) int32 numpy array of the fine shifts found so far, or with blocks (fed, By, Bx, 2): 16 * the whole-pixel
        pick (shifts(), block_shifts()) plus its refinement in [-8, 8]."""
        self._need_subpixel()
        return self._fine[:self.fed].cpu().numpy()

    def valid(self):
        """((y0, y1), (x0, x1)): the rectangle every frame corrected so far covers with its own pixels."""
        if self.subpixel:
            return valid_rectangle(self.fine_shifts(), self.shape, fine=True, bidi=self.bidi)
        return valid_rectangle(self.shifts() if self.blocks is None else self.block_shifts(), self.shape, bidi=self.bidi)


def _rounded_mean(torch, total, n):
    """floor((2 * sum + n) / (2 * n)) of an int64 tensor: the mean rounded half up, exact."""
    return torch.div(2 * total + n, 2 * n, rounding_mode='floor')


def _widen(torch, chunk, unsigned):
    v = chunk.to(torch.int64)
    return v & 0xffff if unsigned else v


def make_template(frames, max_shift=8, iterations=1, device=None, coarse=None, bidi=0):
    """A template for `frames` (N, H, W) numpy int16 / uint16: the rounded mean floor((2 * sum + N) / (2 N)) of the frames, then
    `iterations` times: register the frames to the template (fill 0) and take the rounded mean of the corrected frames.
    coarse=c: the registration is the wide search (max_shift in [c, 16 c]).  bidi=p: the odd lines of every frame are moved by p
    first (dc_bidi_apply, fill 0), for the first mean as for the registration.  Returns (H, W) of the frames' dtype."""
    if not isinstance(frames, np.ndarray) or frames.ndim != 3 or frames.shape[0] < 1:
        raise ValueError('frames must be a (N, H, W) numpy array with N >= 1, not %s' %
                         (type(frames).__name__ if not isinstance(frames, np.ndarray) else repr(tuple(frames.shape))))
    dtype = _frame_dtype(frames.dtype)
    shape = _check_shape(frames.shape[1:])
    S = _check_max_shift(max_shift, shape) if coarse is None else _check_coarse(coarse, max_shift, shape)[1]
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or iterations < 0:
        raise ValueError('iterations must be an integer >= 0, not %r' % (iterations,))
    bidi = _check_bidi(bidi, shape)
    torch, _, L, dev = _open_device(device, 'make_template')
    N, (H, W) = int(frames.shape[0]), shape
    uns = dtype == np.dtype(np.uint16)
    step = max(1, _CHUNK_BYTES // (2 * H * W))
    with torch.cuda.device(dev):
        total = torch.zeros((H, W), dtype=torch.int64, device=dev)
        for a in range(0, N, step):
            chunk = torch.from_numpy(np.array(frames[a:a + step]).view(np.int16)).to(dev)      # a copy: a file mapping is read-only
            if bidi:                          # the first mean is one of corrected lines too
                moved = torch.empty_like(chunk)
                L.dc_bidi_apply(chunk.data_ptr(), int(chunk.shape[0]), bidi, H, W, 0, moved.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
                chunk = moved
            total += _widen(torch, chunk, uns).sum(0)
        tmpl = _rounded_mean(torch, total, N).to(torch.int16).cpu().numpy().view(dtype)
        for _ in range(int(iterations)):
            mc = MotionCorrector(shape, N, dtype, tmpl, max_shift=S, fill=0, device=dev, chunk_frames=step, coarse=coarse, bidi=bidi)
            total.zero_()
            for a in range(0, N, step):
                total += _widen(torch, mc.feed(np.ascontiguousarray(frames[a:a + step])), uns).sum(0)
            tmpl = _rounded_mean(torch, total, N).to(torch.int16).cpu().numpy().view(dtype)
    return tmpl


def estimate_shifts_device(dspath, template=None, max_shift=8, template_frames=200, source='series/raw', device=None,
                           chunk_frames=None, blocks=None, max_dev=3, subpixel=False, coarse=None, bidi=0):
    """(shifts, template): the (T, 2) int32 (dy, dx) of every frame of `source` of a dataset file against `template` -- built
    by make_template (one iteration) from the first min(T, template_frames) frames when none is given.  The recording is
    streamed once, memory-mapped or sliced, never read whole; nothing is corrected here: pass `shifts` to
    summarize_series_device / extract_traces_device.  blocks=(By, Bx): the (T, By, Bx, 2) int32 block shifts within
    +-max_dev of each frame's rigid shift instead (the template is still built rigidly); `shifts=` takes them as they are.
    subpixel=True: the fine shifts in sixteenths of a pixel instead, in the same shapes (the template is still built from
    whole-pixel corrections); `fine_shifts=` takes them as they are.  coarse=c: every search, the template's included, is the
    wide search (max_shift in [c, 16 c], rigid only); the shifts may then exceed 16 pixels, which `shifts=` takes as well.
    bidi=p: the odd lines of every frame are moved by p first, for the template as for the search (estimate_bidi_device finds p);
    pass the same bidi= to whatever takes the shifts."""
    _check_bidi(bidi)
    if coarse is None:
        _check_max_shift(max_shift)
    else:
        _check_coarse(coarse, max_shift, None, blocks)
    subpixel = _check_subpixel(subpixel)
    if blocks is not None:
        _check_blocks(blocks, max_dev)
    if isinstance(template_frames, bool) or not isinstance(template_frames, (int, np.integer)) or template_frames < 1:
        raise ValueError('template_frames must be an integer >= 1, not %r' % (template_frames,))
    frames, close = _open_recording(dspath, source)
    try:
        T = int(frames.shape[0])
        shape = tuple(int(v) for v in frames.shape[1:])
        S = _check_max_shift(max_shift, shape) if coarse is None else _check_coarse(coarse, max_shift, shape, blocks)[1]
        bidi = _check_bidi(bidi, shape)
        if template is None:
            template = make_template(np.asarray(frames[:min(T, int(template_frames))]), max_shift=S, iterations=1, device=device,
                                     coarse=coarse, bidi=bidi)
        if blocks is not None:
            _check_blocks(blocks, max_dev, shape, S)
        mc = MotionCorrector(shape, T, frames.dtype, template, max_shift=S, device=device, chunk_frames=chunk_frames, blocks=blocks,
                             max_dev=max_dev, subpixel=subpixel, coarse=coarse, bidi=bidi)
        for a in range(0, T, mc.chunk_frames):
            mc.feed(np.asarray(frames[a:a + mc.chunk_frames]), correct=False)
        out = mc.fine_shifts() if subpixel else (mc.shifts() if blocks is None else mc.block_shifts())
    finally:
        frames = None                        # a view of the file mapping: released before the file is closed
        close()
    return out, template


class BidiEstimator(_FrameReader):
    """Owns the device state of one recording's scan-phase search: feed() frames in chunks of any size, then offset().  Every
    frame gets its own 2P+1 exact scores (dc_bidi_scores); the offset is picked on the host from their sums over the frames.
    A reader of no declared length, whose resident input is scored in pieces of chunk_frames: the declaration checks, the device,
    the checks of feed()'s argument and the stage are the base's, feed() is its own."""
    _stage_tag, _noun = 'bidi_stage', 'estimator'

    def __init__(self, shape, dtype, max_offset=8, device=None, chunk_frames=None):
        # ---- everything that can be wrong with the arguments is a ValueError before the library or the GPU is touched ----
        self._declare(shape, None, dtype, chunk_frames)
        self.max_offset = _check_bidi_radius(max_offset, self.shape)
        if self.shape[0] * self.shape[1] > (1 << 28):
            raise ValueError('shape must be (H, W) with H * W <= 2**28 for the scan-phase search, not %r' % (self.shape,))
        self._tables = []                  # one (t, 2P+1) int64 tensor per piece, in order
        self._open(device, 'BidiEstimator')
        self._constructed()

    def feed(self, frames):
        """The next frames, any t >= 1: a (t, H, W) numpy array or memmap of the recording's dtype (staged through two pinned
        slots), or a contiguous (t, H, W) torch.int16 tensor on the estimator's device holding the recording's bits (read in
        place).  Their scores become rows [fed, fed + t) of scores()."""
        on_device = self._check_frames(frames)
        t = int(frames.shape[0])
        if t < 1:
            raise ValueError('frames must hold at least one frame')
        torch = self._torch
        H, W = self.shape
        P = self.max_offset
        with torch.cuda.device(self.device):
            main = self._stream()
            main.wait_event(self._ready)
            st = main.cuda_stream

            def piece(fp, tc):
                table = torch.empty((tc, 2 * P + 1), dtype=torch.int64, device=self.device)      # fully written by the launch
                self.L.dc_bidi_scores(fp, self._unsigned, tc, H, W, P, table.data_ptr(), st)
                self._tables.append(table)
                self.fed += tc
            if on_device:
                for a in range(0, t, self.chunk_frames):
                    piece(frames.data_ptr() + 2 * a * H * W, min(self.chunk_frames, t - a))
                frames.record_stream(main)
            else:
                self._staged().run(frames, main, piece)
        return self

    def scores(self):
        """(fed, 2P+1) int64 numpy array: the scores of every frame fed so far, index p + P."""
        if not self._tables:
            return np.zeros((0, 2 * self.max_offset + 1), np.int64)
        return self._torch.cat(self._tables).cpu().numpy()

    def totals(self):
        """The 2P+1 sums of the scores over the frames fed, as Python ints (a sum over frames need not fit 64 bits)."""
        sc = self.scores()
        return [sum(int(v) for v in sc[:, k]) for k in range(sc.shape[1])]

    def offset(self):
        """The offset that minimises (total, p^2, p): pass it as bidi=."""
        if self.fed < 1:
            raise ValueError('offset() before any frame was fed')
        return pick_bidi(self.totals())


def estimate_bidi_device(dspath, max_offset=8, frames=200, source='series/raw', device=None):
    """(offset, totals): the scan-phase offset of `source` of a dataset file, searched within +-max_offset over its first
    min(T, frames) frames (frames=None: all of them), and the 2P+1 totals it was picked from (Python ints, index p + P).  The
    recording is memory-mapped or sliced, never read whole.  Pass the offset as bidi= to MotionCorrector, estimate_shifts_device
    and every reader of the recording."""
    _check_bidi_radius(max_offset)
    if frames is not None and (isinstance(frames, bool) or not isinstance(frames, (int, np.integer)) or frames < 1):
        raise ValueError('frames must be None or an integer >= 1, not %r' % (frames,))
    series, close = _open_recording(dspath, source)
    try:
        T = int(series.shape[0])
        n = T if frames is None else min(T, int(frames))
        shape = tuple(int(v) for v in series.shape[1:])
        est = BidiEstimator(shape, series.dtype, max_offset=max_offset, device=device,
                            chunk_frames=min(n, max(1, _CHUNK_BYTES // (2 * max(1, shape[0] * shape[1])))))
        for a in range(0, n, est.chunk_frames):
            est.feed(np.asarray(series[a:min(n, a + est.chunk_frames)]))
        totals = est.totals()
    finally:
        series = None                        # a view of the file mapping: released before the file is closed
        close()
    return pick_bidi(totals), totals
