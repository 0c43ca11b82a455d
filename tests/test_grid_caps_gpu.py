"""Every capped-grid kernel of the recording pipeline past its cap (DESIGN.md 4f-caps has the table): csrc/motion.hip,
csrc/traces.hip and csrc/dff.hip clamp a grid dimension (65535 frames or tiles, 4096 x 256 groups, 2^20 items, 1024 x 256 zeroed
values) and let a workgroup stride over the rest, and every other module of the suite stays on the first trip.  Here each entry
point runs a launch whose second (or third) trip carries real work, against the oracles the first-trip tests use: _motion_ref,
_motion_block_ref, _motion_sub_ref, _motion_wide_ref, _dff_ref.  Every comparison is equality; every output buffer is pre-filled
with garbage and has guard elements around it.

The long recordings are periodic (tests/_gridcaps.py): frame f is base[f % 37], likewise every per-frame table, so the oracle is
evaluated on 37 items and indexed; 37 divides no stride, so a kernel that takes the wrong frame on a later trip gives another
answer.  The recordings are expanded, and the results compared, on the device."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _dff_ref as dref               # noqa: E402
import _gridcaps as gc                # noqa: E402
import _motion_block_ref as bref      # noqa: E402
import _motion_ref as ref             # noqa: E402
import _motion_sub_ref as sref        # noqa: E402
import _motion_wide_ref as wref       # noqa: E402

GARBAGE = -0x0123456789abcdef
I32_MAX = 2 ** 31 - 1
LIM = 2 ** 62 - 1
GUARD = 8
K, TWO, THREE = gc.K, gc.TWO_TRIPS, gc.THREE_TRIPS
FILLS = {torch.int64: GARBAGE, torch.int32: 12345, torch.int16: 0x5a5a, torch.float32: -7.25}


@pytest.fixture(autouse=True)
def _release_device_memory():
    """The buffers here reach a few hundred MB: hand them back, so that one test's cached blocks do not add to the next one's."""
    yield
    torch.cuda.empty_cache()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    """A numpy array on the device; 16-bit frames as their int16 bits."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32))).cuda()


def _periodic(base, n):
    """n items on the device, item f = base[f % K] (the index is tests/_gridcaps.rows: checked on the CPU)."""
    return _dev(base)[torch.from_numpy(gc.rows(n)).cuda()].contiguous()


def _uns(dtype):
    return int(np.dtype(dtype) == np.dtype(np.uint16))


def _rand(rs, shape, dtype):
    info = np.iinfo(dtype)
    return rs.randint(info.min, info.max + 1, size=shape).astype(dtype)


class _Out(object):
    """n output elements inside a garbage-prefilled buffer with GUARD elements on both sides; odd: `out` starts that many elements
    further into its allocation (off 16-byte alignment for 16-bit outputs).  get() checks that only the n elements changed."""

    def __init__(self, n, dtype, odd=0):
        self.n, self.lead, self.fill = n, GUARD + odd, FILLS[dtype]
        self.buf = torch.full((self.lead + n + GUARD,), self.fill, dtype=dtype, device='cuda')
        self.ptr = self.buf.data_ptr() + self.lead * self.buf.element_size()
        assert (self.ptr % 16 == 0) == (odd * self.buf.element_size() % 16 == 0)

    def get(self, *shape):
        torch.cuda.synchronize()
        a, b = self.buf[:self.lead], self.buf[self.lead + self.n:]
        assert bool((a == self.fill).all()) and bool((b == self.fill).all()), 'a guard element was written'
        return self.buf[self.lead:self.lead + self.n].view(*shape)


def _same(got, want, tag):
    """Equality of two device tensors (floats: of their bits); the failure names how much differs and where it starts."""
    if not torch.is_tensor(want):
        want = _dev(want)
    if got.dtype == torch.float32:
        got, want = got.view(torch.int32), want.view(torch.int32)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    if not torch.equal(got, want):
        bad = (got != want).reshape(got.shape[0], -1).any(dim=1).nonzero().flatten()
        raise AssertionError('%s: %d of %d items differ, the first is item %d' % (tag, len(bad), got.shape[0], int(bad[0])))


def _want(base_result, n):
    """The oracle's result on the K base items, indexed by f % K, on the device."""
    return _periodic(np.asarray(base_result), n)


# ---- 1. dc_motion_ssd: frames beyond 65535, the zero kernel beyond 1024 x 256 ------------------------------------------------------
# The interior is 2 rows x 10 columns in all four: one full lane of 8 pixels and a ragged lane of 2.  S = 1, 5, 9 run on the
# <4, 8>, <8, 8> and <16, 4> instantiations.  Each table holds more than 262144 scores, so the garbage they start from is cleared
# by the zero kernel's later trips or not at all.
@pytest.mark.parametrize('S,H,W,dtype,tc', [(1, 4, 12, np.int16, THREE), (1, 4, 12, np.uint16, THREE), (5, 12, 20, np.int16, TWO),
                                            (9, 20, 28, np.uint16, TWO)])
def test_scores_of_frames_beyond_the_grid(dclib, S, H, W, dtype, tc):
    rs = np.random.RandomState(100 + S)
    assert (H - 2 * S, W - 2 * S) == (2, 10)
    base, tmpl = gc.base_frames(rs, (H, W), dtype), _rand(rs, (H, W), dtype)
    nd = 2 * S + 1
    assert tc * nd * nd > gc.ZERO_CAP
    frames, dt = _periodic(base, tc), _dev(tmpl)
    out = _Out(tc * nd * nd, torch.int64)
    dclib.dc_motion_ssd(frames.data_ptr(), _uns(dtype), tc, dt.data_ptr(), H, W, S, out.ptr, _st())
    _same(out.get(tc, nd, nd), _want(ref.scores(base, tmpl, S), tc), 'scores')


# ---- 2. dc_motion_ssd_around ---------------------------------------------------------------------------------------------------
def _centre_rows(rs, lim):
    """K rows of centres: (0, 0), the corners, rows the device must clamp (|mult * row| > S - D), the int32 extremes, random ones."""
    named = [(0, 0), (1, -1), (-1, 1), (1, 1), (-1, -1), (2, 0), (-1, 0), (0, -2), (0, 1), (-5, 7), (I32_MAX, -I32_MAX),
             (-2 ** 31, I32_MAX), (0, -2 ** 31)]
    more = [tuple(int(v) for v in rs.randint(-lim, lim + 1, size=2)) for _ in range(K - len(named))]
    return np.array(named + more, np.int64)


@pytest.mark.parametrize('dtype', [np.int16, np.uint16])
def test_window_scores_of_frames_beyond_the_grid(dclib, dtype):
    S, D, mult, H, W, tc = 3, 1, 2, 8, 16, TWO
    rs = np.random.RandomState(200)
    base, tmpl, rows = gc.base_frames(rs, (H, W), dtype), _rand(rs, (H, W), dtype), _centre_rows(rs, 3)
    ctr = wref.centres(rows, mult, S, D)
    assert (np.abs(mult * rows) > S - D).any() and len({tuple(c) for c in ctr.tolist()}) == 9           # every clamped centre occurs
    nd = 2 * D + 1
    frames, dt, dr = _periodic(base, tc), _dev(tmpl), _periodic(rows.astype(np.int32), tc)
    out = _Out(tc * nd * nd, torch.int64)
    dclib.dc_motion_ssd_around(frames.data_ptr(), _uns(dtype), tc, dt.data_ptr(), H, W, S, D, dr.data_ptr(), mult, out.ptr, _st())
    _same(out.get(tc, nd, nd), _want(wref.window_scores(base, tmpl, S, D, rows, mult), tc), 'window scores')


# ---- 3. dc_motion_pick, dc_motion_pick_around ------------------------------------------------------------------------------------
def _tied_tables(rs, shape):
    """K fabricated score tables (K, ...) + shape: wide-ranging, heavily tied, constant and with a far strict minimum."""
    t = (rs.randint(0, 2 ** 31, size=(K,) + shape).astype(np.int64) << 31) | rs.randint(0, 2 ** 31, size=(K,) + shape)
    t[::3] >>= 40
    t[1::4] = rs.randint(0, 3, size=t[1::4].shape)       # heavily tied
    t[2] = LIM
    t[5] = 10 ** 6
    t[5].reshape(-1)[-1] = 9                             # a strict minimum in the last entry
    return t


def test_picks_of_frames_beyond_the_grid(dclib):
    S, tc = 2, THREE
    rs = np.random.RandomState(300)
    base = _tied_tables(rs, (5, 5))
    tables = _periodic(base, tc)
    shifts, best = _Out(tc * 2, torch.int32), _Out(tc, torch.int64)
    dclib.dc_motion_pick(tables.data_ptr(), tc, S, shifts.ptr, best.ptr, _st())
    want = ref.pick(base)
    assert len({tuple(r) for r in want.tolist()}) > 8
    _same(shifts.get(tc, 2), _want(want, tc), 'shifts')
    _same(best.get(tc), _want(base.reshape(K, -1).min(axis=1), tc), 'best')


def test_window_picks_of_frames_beyond_the_grid(dclib):
    S, D, mult, tc = 6, 2, 2, THREE
    rs = np.random.RandomState(301)
    base, rows = _tied_tables(rs, (5, 5)), _centre_rows(rs, 4)
    w_shifts, w_best, w_fine = wref.pick_around(base, rows, mult, S)
    assert (w_fine != 16 * w_shifts).any() and (np.abs(mult * rows) > S - D).any()
    tables, dr = _periodic(base, tc), _periodic(rows.astype(np.int32), tc)
    shifts, best, fine = _Out(tc * 2, torch.int32), _Out(tc, torch.int64), _Out(tc * 2, torch.int32)
    dclib.dc_motion_pick_around(tables.data_ptr(), dr.data_ptr(), mult, tc, S, D, shifts.ptr, best.ptr, fine.ptr, _st())
    _same(shifts.get(tc, 2), _want(w_shifts, tc), 'shifts')
    _same(best.get(tc), _want(w_best, tc), 'best')
    _same(fine.get(tc, 2), _want(w_fine, tc), 'fine')


# ---- 4. dc_motion_apply, dc_motion_apply_sub: frames beyond 65535 ------------------------------------------------------------------
# H W = 15 is odd: the first value of frame t lies (15 t) & 7 values off a group of 8, which walks through every residue, and the
# groups straddle frames.  odd = 3: `out` off 16-byte alignment (what MotionCorrector does for every chunk after an odd one).
SMALL = (3, 5)


def _small_shifts(rs, H, W, fine):
    """K shifts (whole pixels, or sixteenths): inside, on the edge of and beyond the frame, the int32 extremes, random ones."""
    q = 16 if fine else 1
    named = [(0, 0), (q, -q), (-q, q), (q * (H - 1), q * (W - 1)), (q * (1 - H), q * (1 - W)), (q * H, 0), (0, -q * W), (0, q * W),
             (-q * H, 0), (I32_MAX, 0), (0, -2 ** 31), (-2 ** 31, I32_MAX)]
    if fine:
        named += [(1, -1), (15, -15), (17, -17), (37, 0), (0, 37), (-40, 23), (8, 8), (16 * (H - 1) + 1, 0), (0, -16 * W - 1)]
    more = [(int(rs.randint(-q * H, q * H + 1)), int(rs.randint(-q * W, q * W + 1))) for _ in range(K - len(named))]
    return np.array(named + more, np.int64)


@pytest.mark.parametrize('odd', [0, 3])
def test_moved_frames_beyond_the_grid(dclib, odd):
    (H, W), tc, fill = SMALL, THREE, -2
    rs = np.random.RandomState(400)
    base, shifts = gc.base_frames(rs, (H, W), np.int16), _small_shifts(rs, H, W, False)
    frames, ds = _periodic(base, tc), _periodic(shifts.astype(np.int32), tc)
    out = _Out(tc * H * W, torch.int16, odd)
    dclib.dc_motion_apply(frames.data_ptr(), tc, ds.data_ptr(), H, W, fill, out.ptr, _st())
    _same(out.get(tc, H, W), _want(ref.apply(base, shifts, fill), tc), 'moved frames')


@pytest.mark.parametrize('odd', [0, 3])
@pytest.mark.parametrize('dtype,fill', [(np.int16, -2), (np.uint16, 48879)])
def test_interpolated_frames_beyond_the_grid(dclib, dtype, fill, odd):
    (H, W), tc = SMALL, THREE
    rs = np.random.RandomState(401)
    base, fine = gc.base_frames(rs, (H, W), dtype), _small_shifts(rs, H, W, True)
    frames, ds = _periodic(base, tc), _periodic(fine.astype(np.int32), tc)
    out = _Out(tc * H * W, torch.int16, odd)
    dclib.dc_motion_apply_sub(frames.data_ptr(), _uns(dtype), tc, ds.data_ptr(), H, W, fill, out.ptr, _st())
    _same(out.get(tc, H, W), _want(sref.apply_sub(base, fine, fill), tc), 'interpolated frames')


# ---- 5. dc_motion_apply, dc_motion_apply_sub: groups beyond 4096 x 256 -------------------------------------------------------------
# Two frames of 2051 x 4099: 8 407 049 values each, more than the 8 388 608 the x grid covers in one trip, so the groups that hold
# output rows 2046 .. 2050 are second-trip (tests/test_grid_caps.py).  The whole-pixel move is compared everywhere.  The
# interpolation is compared on two bands of output rows: the top [0, 8) and the bottom [2043, 2051), which holds every second-trip
# group; the oracle sees the band's rows and a margin of 4 source rows, more than the shifts' |floor(sy / 16)| + 1 = 3.
@pytest.fixture(scope='module')
def big_frames():
    rs = np.random.RandomState(500)
    return _rand(rs, (2, gc.BIG_H, gc.BIG_W), np.uint16)


def test_moved_groups_beyond_the_grid(dclib, big_frames):
    tc, H, W = big_frames.shape
    shifts = np.array([(2, -3), (-1, 5)], np.int64)
    out = _Out(tc * H * W, torch.int16)
    df, ds = _dev(big_frames), _i32(shifts)
    dclib.dc_motion_apply(df.data_ptr(), tc, ds.data_ptr(), H, W, 48879, out.ptr, _st())
    got = out.get(tc, H, W)
    want = ref.apply(big_frames, shifts, 48879)
    lo, hi = gc.apply_second_trip_rows(H, W, tc)
    _same(got[:, lo:hi + 1].reshape(-1, W), want[:, lo:hi + 1].reshape(-1, W), 'second-trip rows')
    _same(got.reshape(-1, W), want.reshape(-1, W), 'rows')


def test_interpolated_groups_beyond_the_grid(dclib, big_frames):
    tc, H, W = big_frames.shape
    fine = np.array([(32, -48), (37, -23)], np.int64)    # one whole-pixel, one fractional: floor(sy / 16) = 2 in both
    band, margin = gc.BIG_BAND, 4
    assert gc.apply_second_trip_rows(H, W, tc)[0] >= H - band and (np.abs(fine[:, 0] // 16) + 1 < margin).all()
    out = _Out(tc * H * W, torch.int16)
    df, ds = _dev(big_frames), _i32(fine)
    dclib.dc_motion_apply_sub(df.data_ptr(), 1, tc, ds.data_ptr(), H, W, 7, out.ptr, _st())
    got = out.get(tc, H, W)
    # a band's oracle: the interpolation of the band's source rows alone; its rows away from the cut are the whole frame's
    top = sref.apply_sub(big_frames[:, :band + margin], fine, 7)[:, :band]
    bottom = sref.apply_sub(big_frames[:, H - band - margin:], fine, 7)[:, margin:]
    assert (top != 7).any() and (bottom[:, :band - 3] != 7).any() and (bottom[:, band - 2:] == 7).all()       # sy > 32: the last rows fill
    _same(got[:, :band].reshape(-1, W), top.reshape(-1, W), 'top rows')
    _same(got[:, H - band:].reshape(-1, W), bottom.reshape(-1, W), 'bottom rows')


# ---- 6. dc_motion_block_ssd ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,D,By,Bx,H,W,dtype', [(1, 1, 2, 2, 10, 12, np.int16), (0, 5, 1, 1, 14, 14, np.uint16)])
def test_block_scores_of_frames_beyond_the_grid(dclib, S, D, By, Bx, H, W, dtype):
    tc = TWO
    rs = np.random.RandomState(600 + D)
    base, tmpl = gc.base_frames(rs, (H, W), dtype), _rand(rs, (H, W), dtype)
    rigid = rs.randint(-S - 2, S + 3, size=(K, 2)).astype(np.int64)
    rigid[:3] = [(1000, -1000), (-2 ** 31, I32_MAX), (S, -S)]
    assert (np.abs(rigid) > S).any()
    nd = 2 * D + 1
    frames, dt, dr = _periodic(base, tc), _dev(tmpl), _periodic(rigid.astype(np.int32), tc)
    out = _Out(tc * By * Bx * nd * nd, torch.int64)
    dclib.dc_motion_block_ssd(frames.data_ptr(), _uns(dtype), tc, dt.data_ptr(), H, W, S, D, By, Bx, dr.data_ptr(), out.ptr, _st())
    _same(out.get(tc, By, Bx, nd, nd), _want(bref.block_scores(base, tmpl, S, D, By, Bx, rigid), tc), 'block scores')


# ---- 7. dc_motion_block_pick: items beyond 2^20 ------------------------------------------------------------------------------------
def test_block_picks_of_items_beyond_the_grid(dclib):
    S, D, By, Bx, tc = 3, 1, 4, 4, TWO
    assert tc * By * Bx > gc.ITEM_CAP
    rs = np.random.RandomState(700)
    base = _tied_tables(rs, (By, Bx, 3, 3))
    rigid = rs.randint(-S - 2, S + 3, size=(K, 2)).astype(np.int64)
    rigid[:2] = [(77, -5), (-2 ** 31, I32_MAX)]
    want_bs, want_best = bref.block_pick(base, rigid, S)
    tables, dr = _periodic(base, tc), _periodic(rigid.astype(np.int32), tc)
    bs, best = _Out(tc * By * Bx * 2, torch.int32), _Out(tc * By * Bx, torch.int64)
    dclib.dc_motion_block_pick(tables.data_ptr(), dr.data_ptr(), tc, By, Bx, S, D, bs.ptr, best.ptr, _st())
    _same(bs.get(tc, By, Bx, 2), _want(want_bs, tc), 'block shifts')
    _same(best.get(tc, By, Bx), _want(want_best, tc), 'best')


# ---- 8. dc_motion_warp, dc_motion_warp_sub -----------------------------------------------------------------------------------------
WARP = (5, 11, 2, 3)                  # H, W, By, Bx: H W = 55 is odd, as in 4


def _block_shifts(rs, H, W, By, Bx, fine):
    q = 16 if fine else 1
    bs = rs.randint(-3 * q, 3 * q + 1, size=(K, By, Bx, 2)).astype(np.int64)
    bs[1] = (q * H, 0)                                   # all fill
    bs[2, :, 1] = (0, -q * W)                            # the middle column of blocks leaves the frame
    bs[3] = 0
    bs[4, 0, 0] = (I32_MAX, -2 ** 31)
    return bs


@pytest.mark.parametrize('odd', [0, 1])
def test_warped_frames_beyond_the_grid(dclib, odd):
    (H, W, By, Bx), tc, fill = WARP, THREE, -2
    rs = np.random.RandomState(800)
    base, bs = gc.base_frames(rs, (H, W), np.int16), _block_shifts(rs, H, W, By, Bx, False)
    frames, ds = _periodic(base, tc), _periodic(bs.astype(np.int32), tc)
    out = _Out(tc * H * W, torch.int16, odd)
    dclib.dc_motion_warp(frames.data_ptr(), tc, ds.data_ptr(), By, Bx, H, W, fill, out.ptr, _st())
    _same(out.get(tc, H, W), _want(bref.warp(base, bs, fill), tc), 'warped frames')


@pytest.mark.parametrize('dtype,fill,odd', [(np.int16, -2, 0), (np.uint16, 48879, 1)])
def test_interpolated_warp_beyond_the_grid(dclib, dtype, fill, odd):
    (H, W, By, Bx), tc = WARP, THREE
    rs = np.random.RandomState(801)
    base, fbs = gc.base_frames(rs, (H, W), dtype), _block_shifts(rs, H, W, By, Bx, True)
    frames, ds = _periodic(base, tc), _periodic(fbs.astype(np.int32), tc)
    out = _Out(tc * H * W, torch.int16, odd)
    dclib.dc_motion_warp_sub(frames.data_ptr(), _uns(dtype), tc, ds.data_ptr(), By, Bx, H, W, fill, out.ptr, _st())
    _same(out.get(tc, H, W), _want(sref.warp_sub(base, fbs, fill), tc), 'interpolated warp')


# ---- 9. dc_roi_trace_accumulate: tiles beyond 65535, the zero kernel ---------------------------------------------------------------
TRACE_SHAPE = (2, 3)
# (row_off, row_pix, row_roi, the ROIs' pixel lists): every CSR row an ROI (plain stores); three rows that feed two ROIs (atomics
# into columns the call has zeroed)
CSR = {'stores': ([0, 4, 6], [0, 1, 4, 5, 2, 3], None, [[0, 1, 4, 5], [2, 3]]),
       'atomics': ([0, 2, 5, 6], [0, 1, 2, 3, 4, 5], [0, 1, 0], [[0, 1, 5], [2, 3, 4]])}


@pytest.mark.parametrize('form,dtype', [('stores', np.int16), ('atomics', np.uint16)])
def test_roi_sums_of_tiles_beyond_the_grid(dclib, form, dtype):
    (H, W), tc, t0, pad = TRACE_SHAPE, gc.TRACE_FRAMES, 3, 5
    off, pix, roi, lists = CSR[form]
    S, R, ld = len(off) - 1, len(lists), t0 + tc + pad
    assert roi is None or R * tc > gc.ZERO_CAP
    rs = np.random.RandomState(900)
    base = gc.base_frames(rs, (H, W), dtype)
    frames = _periodic(base, tc)
    sums = torch.full((R, ld), GARBAGE, dtype=torch.int64, device='cuda')
    d_off, d_pix, d_roi = _i32(off), _i32(pix), (_i32(roi) if roi is not None else None)
    dclib.dc_roi_trace_accumulate(frames.data_ptr(), _uns(dtype), tc, t0, d_off.data_ptr(), d_pix.data_ptr(),
                                  d_roi.data_ptr() if roi is not None else None, S, R, sums.data_ptr(), ld, H, W, _st())
    torch.cuda.synchronize()
    assert bool((sums[:, :t0] == GARBAGE).all()) and bool((sums[:, t0 + tc:] == GARBAGE).all()), 'a guard column was written'
    want = gc.roi_sums(base, lists)                      # (R, K)
    _same(sums[:, t0:t0 + tc].t().contiguous(), _want(want.T, tc), 'sums')


# ---- 10. dc_trace_combine, dc_trace_scale, dc_trace_baseline: chunks / tiles beyond 65535 -----------------------------------------
@pytest.fixture(scope='module')
def long_trace():
    """(DFF_FRAMES,) int64 within +-1000, and int64 extremes in the two second-trip tiles (frames from 65535 * 256 on)."""
    rs = np.random.RandomState(1000)
    T = gc.DFF_FRAMES
    x = rs.randint(-1000, 1001, size=T).astype(np.int64)
    first = gc.FRAME_CAP * gc.DFF_TILE
    x[[first + 1, first + 2, first + 255, first + 256, T - 2, T - 1]] = [LIM, -LIM, -LIM, LIM, LIM, -LIM]
    return x


def _row_matrix(rows, pad):
    """(R, T) -> a device matrix of row stride T + pad with garbage behind every row."""
    R, T = len(rows), len(rows[0])
    d = torch.full((R, T + pad), GARBAGE, dtype=torch.int64, device='cuda')
    for r, row in enumerate(rows):
        d[r, :T] = torch.from_numpy(row)
    return d


def test_combine_of_chunks_beyond_the_grid(dclib, long_trace):
    x, T, pad = long_trace, len(long_trace), 4
    ring = np.roll(x, 12345) % 2001 - 1000               # a second row within +-1000
    ca, cb, cc = 3, 5, -7
    small = np.where(np.abs(x) > 1000, x // 4, x)        # 3 x stays inside int64
    d = _row_matrix([small, ring], pad)
    dev = [torch.tensor(v, device='cuda') for v in (np.array([1], np.int32), np.array([ca], np.int64), np.array([cb], np.int64),
                                                    np.array([cc], np.int64))]
    out = _Out(T, torch.int64)
    dclib.dc_trace_combine(d.data_ptr(), T + pad, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), 1, T,
                           out.ptr, _st())
    _same(out.get(1, T).t(), torch.from_numpy(ca * small - cb * ring + cc).cuda()[:, None], 'num')


def test_scale_of_chunks_beyond_the_grid(dclib, long_trace):
    x, T, pad = long_trace, len(long_trace), 1
    d, den = _row_matrix([x], pad), torch.tensor([7], dtype=torch.int64, device='cuda')
    out = _Out(T, torch.float32)
    dclib.dc_trace_scale(d.data_ptr(), T + pad, den.data_ptr(), 1, T, out.ptr, _st())
    _same(out.get(1, T).t(), torch.from_numpy(dref.scale(x[None], np.array([7]))).cuda().t(), 'scaled')


def test_baseline_of_tiles_beyond_the_grid(dclib, long_trace):
    x, T, pad, half, q = long_trace, len(long_trace), 3, 1, 50
    tail = x[None, -1000:]
    assert np.array_equal(gc.baseline_half1(tail, q), dref.baseline(tail, half, q)) and np.abs(tail).max() == LIM
    want_b = gc.baseline_half1(x[None], q)
    want_d = dref.dff(x[None], want_b)
    assert (want_b > 0).any() and (want_b <= 0).any()
    d = _row_matrix([x], pad)
    ob, od = _Out(T, torch.int64), _Out(T, torch.float32)
    dclib.dc_trace_baseline(d.data_ptr(), T + pad, 1, T, half, q, ob.ptr, od.ptr, _st())
    _same(ob.get(1, T).t(), torch.from_numpy(want_b).cuda().t(), 'baseline')
    _same(od.get(1, T).t(), torch.from_numpy(want_d).cuda().t(), 'dff')
    assert bool((d[0, :T] == torch.from_numpy(x).cuda()).all()) and bool((d[0, T:] == GARBAGE).all())      # the input is only read


# ---- through the Python API, with the default chunk_frames: the whole recording is one launch -------------------------------------
API = (8, 16, 2)                      # H, W, max_shift


def _api_oracle(config, base, tmpl):
    """The oracle's tables and corrected frames of the K base frames for one MotionCorrector configuration."""
    S = API[2]
    if config == 'rigid':
        pk = ref.pick(ref.scores(base, tmpl, S))
        return dict(shifts=pk, out=ref.apply(base, pk, 0))
    if config == 'blocks':
        sc = ref.scores(base, tmpl, S)
        pk = ref.pick(sc)
        bsc = bref.block_scores(base, tmpl, S, 1, 1, 2, pk)
        bs, _ = bref.block_pick(bsc, pk, S)
        bfine = sref.block_refine(bsc, pk, bs, S)
        return dict(shifts=pk, block_shifts=bs, fine_shifts=bfine, out=sref.warp_sub(base, bfine, 0))
    r = wref.search(base, tmpl, S, 2)
    return dict(shifts=r['shifts'], coarse_shifts=r['coarse'], out=ref.apply(base, r['shifts'], 0))


CONFIGS = {'rigid': {}, 'blocks': dict(blocks=(1, 2), max_dev=1, subpixel=True), 'coarse': dict(coarse=2)}


@pytest.mark.parametrize('config', sorted(CONFIGS))
def test_motion_corrector_registers_a_long_recording_in_one_launch(config):
    from deep_calcium_amd import MotionCorrector
    H, W, S = API
    tc = TWO
    rs = np.random.RandomState(1100)
    base, tmpl = gc.base_frames(rs, (H, W), np.uint16), _rand(rs, (H, W), np.uint16)
    want = _api_oracle(config, base, tmpl)
    assert len({tuple(r) for r in want['shifts'].tolist()}) > 4
    frames = gc.expand(base, tc)
    runs = []
    for chunk_frames in (None, 64):
        mc = MotionCorrector((H, W), tc, np.uint16, tmpl, max_shift=S, chunk_frames=chunk_frames, **CONFIGS[config])
        assert mc.chunk_frames == (tc if chunk_frames is None else 64)       # None: the default chunk holds the whole recording
        out = mc.feed(frames)
        got = dict(out=out)
        for name in want:
            if name != 'out':
                got[name] = getattr(mc, name + '_device')()[:mc.fed]
        runs.append(got)
    for name in sorted(want):
        _same(runs[0][name], runs[1][name], (config, name, 'one launch against chunks of 64'))
        _same(runs[0][name], _want(want[name], tc), (config, name))


def test_trace_extractor_sums_a_long_recording_in_one_launch():
    from deep_calcium_amd import RoiTraceExtractor
    (H, W), tc = TRACE_SHAPE, gc.TRACE_FRAMES
    rs = np.random.RandomState(1200)
    base = gc.base_frames(rs, (H, W), np.int16)
    lists = CSR['atomics'][3]
    rois = [np.array([divmod(p, W) for p in lst]) for lst in lists]
    frames = gc.expand(base, tc)
    runs = []
    for chunk_frames in (None, 64):
        ext = RoiTraceExtractor((H, W), tc, np.int16, rois, chunk_frames=chunk_frames)
        assert ext.chunk_frames == (tc if chunk_frames is None else 64)
        runs.append(ext.feed(frames).sums_device().t().contiguous())
    _same(runs[0], runs[1], 'one launch against chunks of 64')
    _same(runs[0], _want(gc.roi_sums(base, lists).T, tc), 'sums')
