"""Every recording and trace kernel with an element offset past 2^31 (DESIGN.md 4f-wide has the table, tests/_wideindex.py the
shapes and tests/test_wide_index.py their arithmetic): `r * ld` with ld, or the product, beyond int32 (the row route), `f * H * W`
from frame 131072 of 128 x 128 on (the frame route), and the two capped grids that DESIGN.md 4f-caps had to leave out, whose
crossing shapes need 8 GiB of input.  Everything large is made and compared on the device; the oracles of the first-trip tests see
the 37 base items of a periodic recording (tests/_gridcaps.py), or the two or three short rows of a matrix.  Every comparison is
equality, but the z-score, which keeps the 1 ulp of the header.  A kernel that keeps only 31 bits of an offset stays inside every
allocation here and meets other valid data: another base frame (131072 mod 37 = 18), or the decoy row planted at the masked offset
of a matrix's last row -- so it fails with a wrong number, not a fault.

A test skips only when the device has less free memory than its row of the table asks for."""
import contextlib
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _bidi_ref as biref             # noqa: E402
import _deconv_ar2_ref as a2ref       # noqa: E402
import _deconv_base_ref as bsref      # noqa: E402
import _deconv_ref as dcref           # noqa: E402
import _deconv_search_ref as srref    # noqa: E402
import _dff_ref as dref               # noqa: E402
import _dyn_ref as dyref              # noqa: E402
import _footprints_ref as fpref       # noqa: E402
import _frames_ref as frref           # noqa: E402
import _gridcaps as gc                # noqa: E402
import _merge_ref as mgref            # noqa: E402
import _motion_block_ref as bref      # noqa: E402
import _motion_ref as ref             # noqa: E402
import _motion_sub_ref as sref        # noqa: E402
import _motion_wide_ref as wref       # noqa: E402
import _pair_ref as paref             # noqa: E402
import _tbin_ref as tbref             # noqa: E402
import _weighted_ref as wtref         # noqa: E402
import _wideindex as wi               # noqa: E402
from test_series_gpu import _ulps, _xy_ref            # noqa: E402  the cross sums and the float32 distance of the series tests
from test_traces_gpu import _zscore_ref               # noqa: E402  the exact z-score of the trace tests

K = wi.K
GARBAGE = -0x0123456789abcdef
PATTERN = 0x5a5a
I32_MAX = 2 ** 31 - 1
LIM = 2 ** 62 - 1
GUARD = 8
CANARY = -77.25
FILLS = {torch.int64: GARBAGE, torch.int32: 12345, torch.int16: PATTERN, torch.float32: float('nan'), torch.float64: float('nan')}
H, W = wi.FRAME_HW
TC = wi.FRAME_TC
CHUNK = 1 << 25                       # elements compared at a time: the comparison's own temporaries stay at 32 MiB
ROW_IDS = ['A', 'B']


# ---- memory: the skip rule, the budget, the release -----------------------------------------------------------------------------
@contextlib.contextmanager
def _budget(*names):
    """The test of the table rows `names`: skips when the device has less free memory than the largest of them asks for (plus 1 GiB),
    prints the peak it reached above what other tests' fixtures still hold, holds that to the row, and hands everything back."""
    need = max(wi.TABLE[n][2] for n in names)
    assert need <= wi.BUDGET
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info()[0]
    if free < need + wi.GiB:
        pytest.skip('%d bytes of device memory are free, the test needs %d and 1 GiB to spare' % (free, need))
    torch.cuda.reset_peak_memory_stats()
    held = torch.cuda.memory_allocated()                 # module fixtures of tests that ran before: not this test's
    try:
        yield
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - held
        print('%s: peak %.3f GiB of %.3f GiB in the table, %.1f GiB were free' % (names[0], peak / wi.GiB, need / wi.GiB, free / wi.GiB))
        assert peak <= need, (names, peak, need)
    finally:
        torch.cuda.empty_cache()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    """A numpy array on the device; 16-bit frames as their int16 bits."""
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32))).cuda()


def _idx(n):
    """f % K for the n items of a periodic recording, on the device (tests/_gridcaps.rows is the same on the host)."""
    return torch.arange(n, device='cuda') % K


def _periodic(base, idx):
    """Item f = base[f % K], on the device."""
    assert len(base) == K
    return _dev(base)[idx]


def _uns(dtype):
    return int(np.dtype(dtype) == np.dtype(np.uint16))


def _rand(rs, shape, dtype):
    info = np.iinfo(dtype)
    return rs.randint(info.min, info.max + 1, size=shape).astype(dtype)


def _all(t, value):
    """Every element of a device tensor of any size equals `value` (NaN: is NaN); in pieces of CHUNK elements, one flag, one sync."""
    flat = t.reshape(-1)
    ok = torch.ones((), dtype=torch.bool, device='cuda')
    for lo in range(0, flat.numel(), CHUNK):
        piece = flat[lo:lo + CHUNK]
        ok &= (torch.isnan(piece) if isinstance(value, float) and math.isnan(value) else piece == value).all()
    return bool(ok)


def _same(got, want, tag):
    """Equality of two device tensors of any size (floats: of their bits), in pieces of CHUNK elements along the first axis; the
    failure names how many items differ and the first of them."""
    if not torch.is_tensor(want):
        want = _dev(np.asarray(want))
    if got.dtype in (torch.float32, torch.float64):
        view = torch.int32 if got.dtype == torch.float32 else torch.int64
        got, want = got.contiguous().view(view), want.contiguous().view(view)
    assert got.shape == want.shape and got.dtype == want.dtype, (tag, got.shape, want.shape, got.dtype, want.dtype)
    n = got.shape[0]
    per = max(1, got.numel() // max(n, 1))
    step = max(1, CHUNK // per)
    bad, first = 0, None
    for lo in range(0, n, step):
        a, b = got[lo:lo + step], want[lo:lo + step]
        if not torch.equal(a, b):
            rows = (a != b).reshape(a.shape[0], -1).any(dim=1).nonzero().flatten()
            bad += len(rows)
            first = lo + int(rows[0]) if first is None else first
    assert bad == 0, '%s: %d of %d items differ, the first is item %d' % (tag, bad, n, first)


class _Out(object):
    """n output elements inside a pre-filled buffer with GUARD elements on both sides; odd: `out` starts that many elements further
    into its allocation (for 16-bit outputs: not a multiple of 8 values, off 16-byte alignment).  get() checks the guards."""

    def __init__(self, n, dtype, odd=0):
        self.n, self.lead, self.fill = n, GUARD + odd, FILLS[dtype]
        self.buf = torch.full((self.lead + n + GUARD,), self.fill, dtype=dtype, device='cuda')
        self.ptr = self.buf.data_ptr() + self.lead * self.buf.element_size()
        assert (self.ptr % 16 == 0) == (odd * self.buf.element_size() % 16 == 0)

    def get(self, *shape):
        torch.cuda.synchronize()
        assert _all(self.buf[:self.lead], self.fill) and _all(self.buf[self.lead + self.n:], self.fill), 'a guard element was written'
        return self.buf[self.lead:self.lead + self.n].view(*shape)


class _Rows(object):
    """The rows of a matrix at stride ld in one device buffer of (R - 1) ld + T elements (tests/_wideindex.ROW_CASES), everything
    else pre-filled (NaN, or GARBAGE for integers).  An input (rows given): behind row 0, wi.decoy_offset(case) further values of
    `decoy` continue it, so that the T elements at the masked offset of the last row are all valid data, and none of them the last
    row's.  An output (rows None): written() checks that nothing but the columns [t0, t0 + tc) of every row changed."""

    def __init__(self, case, dtype, rows=None, decoy=None):
        self.case = case
        self.R, self.ld, self.T = case
        self.fill = FILLS[dtype]
        self.buf = torch.full((wi.row_elements(case),), self.fill, dtype=dtype, device='cuda')
        self.off = wi.decoy_offset(case)
        assert 0 < self.off < self.ld - self.T and wi.last_row_offset(case) >= wi.LINE
        if rows is not None:
            rows = np.ascontiguousarray(rows)
            assert rows.shape == (self.R, self.T) and len(decoy) == self.off
            for r in range(self.R):
                self.row(r)[:] = torch.from_numpy(rows[r]).cuda()
            self.buf[self.T:self.T + self.off] = torch.from_numpy(np.ascontiguousarray(decoy).astype(rows.dtype)).cuda()
            masked = self.buf[self.off:self.off + self.T]
            assert _all(masked, self.fill) is False and not torch.equal(masked, self.row(self.R - 1))
            self.planted = self.T + self.off
        else:
            self.planted = 0
        self.ptr = self.buf.data_ptr()

    def row(self, r, t0=0, tc=None):
        lo = r * self.ld + t0
        return self.buf[lo:lo + (self.T if tc is None else tc)]

    def matrix(self, t0=0, tc=None):
        return torch.stack([self.row(r, t0, tc) for r in range(self.R)])

    def untouched(self, rows, decoy):
        """An input after the call: the rows and the decoy hold what they held, everything else the fill."""
        torch.cuda.synchronize()
        for r in range(self.R):
            assert torch.equal(self.row(r), torch.from_numpy(np.ascontiguousarray(rows[r])).cuda()), ('row %d was written' % r)
        self.written(0, self.T, lead=self.planted)

    def written(self, t0, tc, lead=None):
        """Nothing outside the columns [t0, t0 + tc) of the rows holds anything but the fill (lead: the first row's span)."""
        torch.cuda.synchronize()
        edge = 0
        for r in range(self.R):
            lo = r * self.ld + t0
            assert _all(self.buf[edge:lo], self.fill), 'an element in front of row %d was written' % r
            edge = lo + tc if (lead is None or r > 0) else lead
        assert _all(self.buf[edge:], self.fill), 'an element behind the last row was written'


def _int_rows(case, seed, lim=1000):
    """R different rows of T int64 values within +-lim, and the decoy values that continue row 0."""
    R, _, T = case
    rs = np.random.RandomState(seed)
    rows = rs.randint(-lim, lim + 1, size=(R, T)).astype(np.int64)
    decoy = rs.randint(-lim, lim + 1, size=wi.decoy_offset(case)).astype(np.int64)
    return rows, decoy


# =================================================================================================================================
# The row route, int64 rows: csrc/dff.hip, csrc/traces.hip, csrc/footprints.hip, csrc/trace_pairs.hip
# =================================================================================================================================
def _row_case(name):
    return wi.ROW_CASES[name]


@pytest.mark.parametrize('case', ROW_IDS)
def test_combine_of_rows_beyond_the_line(dclib, case):
    """num[r] = ca[r] sums[r] - cb[r] sums[np_row[r]] + cc[r]: the last row is both a first and a second term."""
    case = _row_case(case)
    R, ld, T = case
    with _budget('dc_trace_combine'):
        rows, decoy = _int_rows(case, 10)
        rows[R - 1, [1, T - 1]] = [LIM // 8, -LIM // 8]
        m = _Rows(case, torch.int64, rows, decoy)
        np_row = np.array([R - 1] + [-1] * (R - 2) + [0], np.int32)          # row 0 takes the last row off, the last row takes row 0
        ca, cb, cc = np.arange(3, 3 + R, dtype=np.int64), np.arange(5, 5 + R, dtype=np.int64), np.arange(-7, -7 + R, dtype=np.int64)
        d = [_dev(a) for a in (np_row, ca, cb, cc)]
        out = _Out(R * T, torch.int64)
        dclib.dc_trace_combine(m.ptr, ld, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), R, T, out.ptr, _st())
        want = np.stack([ca[r] * rows[r] - (cb[r] * rows[np_row[r]] if np_row[r] >= 0 else 0) + cc[r] for r in range(R)])
        _same(out.get(R, T), want, 'num')
        m.untouched(rows, decoy)


@pytest.mark.parametrize('case', ROW_IDS)
def test_scale_of_rows_beyond_the_line(dclib, case):
    case = _row_case(case)
    R, ld, T = case
    with _budget('dc_trace_scale'):
        rows, decoy = _int_rows(case, 11)
        rows[R - 1, [0, T - 1]] = [LIM, -LIM]
        den = np.array([7, 0, 13][:R - 1] + [11], np.int64)
        m, dd = _Rows(case, torch.int64, rows, decoy), _dev(den)
        out = _Out(R * T, torch.float32)
        dclib.dc_trace_scale(m.ptr, ld, dd.data_ptr(), R, T, out.ptr, _st())
        _same(out.get(R, T), dref.scale(rows, den), 'scaled')
        m.untouched(rows, decoy)


@pytest.mark.parametrize('case', ROW_IDS)
def test_baseline_of_rows_beyond_the_line(dclib, case):
    """Half-width 20, rank 30 %: the window of every frame of the second tile of 256 reaches into the first."""
    case = _row_case(case)
    R, ld, T = case
    half, q = 20, 30
    with _budget('dc_trace_baseline'):
        rows, decoy = _int_rows(case, 12)
        rows[R - 1, [3, 255, 256, T - 1]] = [LIM, -LIM, LIM, -LIM]
        rows[0, 100:140] = 7                                             # ties
        want_b = dref.baseline(rows, half, q)
        want_d = dref.dff(rows, want_b)
        assert (want_b[R - 1] > 0).any() and (want_b[R - 1] <= 0).any()
        m = _Rows(case, torch.int64, rows, decoy)
        ob, od = _Out(R * T, torch.int64), _Out(R * T, torch.float32)
        dclib.dc_trace_baseline(m.ptr, ld, R, T, half, q, ob.ptr, od.ptr, _st())
        _same(ob.get(R, T), want_b, 'baseline')
        _same(od.get(R, T), want_d, 'dff')
        m.untouched(rows, decoy)


@pytest.mark.parametrize('case', ROW_IDS)
def test_finalize_of_rows_beyond_the_line(dclib, case):
    """mean bit-equal to numpy's; zscore within 1 float32 ulp of exact arithmetic, the header's promise."""
    case = _row_case(case)
    R, ld, T = case
    with _budget('dc_roi_trace_finalize'):
        rows, decoy = _int_rows(case, 13, lim=2 ** 40)
        areas = np.array([5, 1, 9][:R - 1] + [3], np.int32)
        m, da = _Rows(case, torch.int64, rows, decoy), _dev(areas)
        mean, z = _Out(R * T, torch.float32), _Out(R * T, torch.float32)
        dclib.dc_roi_trace_finalize(m.ptr, ld, da.data_ptr(), R, T, mean.ptr, z.ptr, _st())
        _same(mean.get(R, T), (rows / areas[:, None]).astype(np.float32), 'mean')
        got, zref = z.get(R, T).cpu().numpy(), _zscore_ref(rows)
        assert np.isfinite(got).all()
        d = _ulps(got, zref)
        print('zscore: max %d ulp' % d.max())
        assert d.max() <= 1, int(d.max())
        m.untouched(rows, decoy)


def _i64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


@pytest.mark.parametrize('case', ROW_IDS)
def test_trace_moments_of_rows_beyond_the_line(dclib, case):
    """rmom = (sum S, the low and the high word of sum S^2) per row; the squares of 2^40-sized sums need the high word."""
    case = _row_case(case)
    R, ld, T = case
    with _budget('dc_roi_trace_moments'):
        rows, decoy = _int_rows(case, 14, lim=2 ** 40)
        m = _Rows(case, torch.int64, rows, decoy)
        rmom = _Out(3 * R, torch.int64)
        dclib.dc_roi_trace_moments(m.ptr, ld, R, T, rmom.ptr, _st())
        want = np.zeros((3, R), np.int64)
        for r in range(R):
            s = [int(v) for v in rows[r]]
            w = sum(v * v for v in s)
            want[:, r] = [sum(s), _i64(w), w >> 64]
        assert (want[2] != 0).all()
        _same(rmom.get(3, R), want, 'rmom')
        m.untouched(rows, decoy)


@pytest.mark.parametrize('seg_len', [0, 64])
@pytest.mark.parametrize('case', ROW_IDS)
def test_pair_moments_of_rows_beyond_the_line(dclib, case, seg_len):
    """Every pair of rows, both orders, the diagonal and a pair that names no row; one segment, and segments of 64 frames."""
    case = _row_case(case)
    R, ld, T = case
    with _budget('dc_trace_pair_moments'):
        rows, decoy = _int_rows(case, 15, lim=2 ** 30)
        pairs = [(i, j) for i in range(R) for j in range(R)] + [(R - 1, R), (-1, 0)]
        m, dp = _Rows(case, torch.int64, rows, decoy), _i32(pairs)
        num = _Out(len(pairs) * 6, torch.int64)
        dclib.dc_trace_pair_moments(m.ptr, ld, R, T, seg_len, dp.data_ptr(), len(pairs), num.ptr, _st())
        want = mgref.moment_words(mgref.moments([[int(v) for v in row] for row in rows], pairs, seg_len))
        _same(num.get(len(pairs), 6), want, 'num')
        m.untouched(rows, decoy)


# =================================================================================================================================
# The row route, float32 / float64 traces: csrc/trace_dyn.hip, csrc/deconv.hip
# =================================================================================================================================
GAMMA = math.exp(-1.0 / 8)
TORCH_OF = {np.float32: torch.float32, np.float64: torch.float64}


def _traces(case, dtype, seed):
    """R different traces -- events on noise, a noiseless spike train, noise around an offset -- and the decoy values; -> also the
    noise each is held to in the searches."""
    R, _, T = case
    rs = np.random.RandomState(seed)
    t = np.arange(T)
    y, sigma = np.zeros((R, T)), np.zeros(R)
    for r in range(R):
        sp = rs.poisson(0.05, T) > 0
        kind = (R - 1 - r) % 3                                           # the last row, the one beyond the line, is the richest
        if kind == 0:
            sigma[r] = 0.2 + 0.1 * r
            y[r] = np.convolve(sp, np.exp(-t / 8.0))[:T] + sigma[r] * (rs.standard_normal(T) + 1.0)
        elif kind == 1:
            y[r] = np.convolve(sp, np.exp(-t / 8.0))[:T]
        else:
            y[r] = 0.25 * rs.standard_normal(T) - 0.2
            sigma[r] = 0.5
    decoy = np.convolve(rs.poisson(0.2, 64) > 0, np.exp(-np.arange(64) / 3.0))[:wi.decoy_offset(case)] + 0.5
    return y.astype(dtype), sigma, decoy.astype(dtype)


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('case', ROW_IDS)
def test_noise_of_rows_beyond_the_line(dclib, case, dtype):
    case = _row_case(case)
    R, ld, T = case
    with _budget('dc_trace_noise'):
        y, _, decoy = _traces(case, dtype, 20)
        m = _Rows(case, TORCH_OF[dtype], y, decoy)
        sigma = _Out(R, torch.float64)
        dclib.dc_trace_noise(m.ptr, int(dtype == np.float64), ld, R, T, sigma.ptr, _st())
        _same(sigma.get(R), dyref.noise(y), 'sigma')
        m.untouched(y, decoy)


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('case', ROW_IDS)
def test_ar1_estimate_of_rows_beyond_the_line(dclib, case, dtype):
    case = _row_case(case)
    R, ld, T = case
    lags = 5
    with _budget('dc_trace_ar1_estimate'):
        y, _, decoy = _traces(case, dtype, 21)
        m = _Rows(case, TORCH_OF[dtype], y, decoy)
        sigma, xc, g = _Out(R, torch.float64), _Out(R * (lags + 1), torch.float64), _Out(R, torch.float64)
        dclib.dc_trace_ar1_estimate(m.ptr, int(dtype == np.float64), ld, R, T, lags, None, sigma.ptr, xc.ptr, g.ptr, _st())
        w_sigma, w_xc, w_g = dyref.estimate(y, lags)
        _same(sigma.get(R), w_sigma, 'sigma')
        _same(xc.get(R, lags + 1), w_xc, 'autocov')
        _same(g.get(R), w_g, 'g_raw')
        m.untouched(y, decoy)


class _Deconv(object):
    """What the ten deconvolution entry points share: the traces (a pointer, ld), the tables (one for all traces, or one row per trace
    at stride ldG), and outputs that are GUARD rows longer than they need be, pre-filled with a canary."""

    def __init__(self, L, y_ptr, ld, R, T, f64, G_ptr, ldG=0, gs=None):
        self.L, self.y, self.ld, self.R, self.T, self.f64 = L, y_ptr, ld, R, T, int(f64)
        self.G, self.ldG = G_ptr, ldG
        self.gs = None if gs is None else _dev(np.ascontiguousarray(gs, np.float64))
        self.gv, self.gp = (GAMMA, None) if gs is None else (0.0, self.gs.data_ptr())
        self.ws = self.full(5 * R * T + GUARD, fill=float('nan'))
        self.ws[5 * R * T:] = CANARY

    def full(self, shape, dtype=torch.float64, fill=None):
        fill = (-7 if dtype == torch.int32 else CANARY) if fill is None else fill
        return torch.full(shape if isinstance(shape, tuple) else (shape,), fill, dtype=dtype, device='cuda')

    def vector(self, x, guard=False):
        a = np.broadcast_to(np.asarray(x, np.float64), (self.R,)).copy()
        return torch.from_numpy(np.concatenate([a, np.full(GUARD, CANARY)]) if guard else a).cuda()

    def outputs(self):
        R, T = self.R, self.T
        self.c, self.s, self.n = self.full((R + GUARD, T)), self.full((R + GUARD, T)), self.full(R + GUARD, torch.int32)

    def check(self, **more):
        torch.cuda.synchronize()
        R = self.R
        for name, a in dict(calcium=self.c, spikes=self.s, pools=self.n, **more).items():
            assert _all(a[R:], -7 if a.dtype == torch.int32 else CANARY), (name, 'written beyond row R')
        assert _all(self.ws[5 * R * self.T:], CANARY)
        out = dict(calcium=self.c[:R].cpu().numpy(), spikes=self.s[:R].cpu().numpy(), pools=self.n[:R].cpu().numpy())
        out.update({k: v[:R].cpu().numpy() for k, v in more.items()})
        return out

    # -- the entry points; each -> a dict like its oracle's ---------------------------------------------------------------------------
    def ar1(self, lam, smin):
        lam, smin = self.vector(lam), self.vector(smin)
        self.outputs()
        self.L.dc_trace_deconv_ar1(self.y, self.f64, self.ld, self.R, self.T, GAMMA, self.G, lam.data_ptr(), smin.data_ptr(), self.ws.data_ptr(),
                                   self.c.data_ptr(), self.s.data_ptr(), self.n.data_ptr(), _st())
        return self.check()

    def each(self, lam, smin):
        lam, smin = self.vector(lam), self.vector(smin)
        self.outputs()
        self.L.dc_trace_deconv_ar1_each(self.y, self.f64, self.ld, self.R, self.T, self.gp, self.G, self.ldG, lam.data_ptr(), smin.data_ptr(),
                                        self.ws.data_ptr(), self.c.data_ptr(), self.s.data_ptr(), self.n.data_ptr(), _st())
        return self.check()

    def base(self, lam, smin, base):
        lam, smin, b = self.vector(lam), self.vector(smin), self.vector(base, True)
        self.outputs()
        self.L.dc_trace_deconv_ar1_base(self.y, self.f64, self.ld, self.R, self.T, self.gv, self.gp, self.G, self.ldG, lam.data_ptr(),
                                        smin.data_ptr(), b.data_ptr(), self.ws.data_ptr(), self.c.data_ptr(), self.s.data_ptr(),
                                        self.n.data_ptr(), _st())
        return self.check(baseline=b)

    def fit(self, lam, smin, base, rounds):
        lam, smin, b = self.vector(lam), self.vector(smin), self.vector(base, True)
        self.outputs()
        self.L.dc_trace_deconv_ar1_fit_base(self.y, self.f64, self.ld, self.R, self.T, self.gv, self.gp, self.G, self.ldG, lam.data_ptr(),
                                            smin.data_ptr(), rounds, self.ws.data_ptr(), self.c.data_ptr(), self.s.data_ptr(),
                                            self.n.data_ptr(), b.data_ptr(), _st())
        return self.check(baseline=b)

    def constrained(self, which, sigma, other, rounds):
        """dc_trace_deconv_ar1_constrained, then its last round alone: dc_trace_deconv_search_step on the state it left."""
        R = self.R
        sigma, other = self.vector(sigma), self.vector(other)
        self.outputs()
        state = self.full(5 * R + GUARD)
        param, rss, status = self.full(R + GUARD), self.full(R + GUARD), self.full(R + GUARD, torch.int32)
        self.L.dc_trace_deconv_ar1_constrained(self.y, self.f64, self.ld, R, self.T, self.gv, self.gp, self.G, self.ldG, which, sigma.data_ptr(),
                                               other.data_ptr(), rounds, self.ws.data_ptr(), state.data_ptr(), self.c.data_ptr(),
                                               self.s.data_ptr(), self.n.data_ptr(), param.data_ptr(), rss.data_ptr(), status.data_ptr(), _st())
        out = self.check(param=param, rss=rss, status=status)
        assert _all(state[5 * R:], CANARY)
        out['target'] = state[3 * R:4 * R].cpu().numpy()
        p2, r2, s2 = param.clone(), self.full(R + GUARD), self.full(R + GUARD, torch.int32)
        self.L.dc_trace_deconv_search_step(self.y, self.f64, self.ld, R, self.T, self.G, self.ldG, self.ws.data_ptr(), self.n.data_ptr(), 1,
                                           state.data_ptr(), p2.data_ptr(), r2.data_ptr(), s2.data_ptr(), _st())
        torch.cuda.synchronize()
        assert _all(r2[R:], CANARY) and _all(s2[R:], -7) and _all(p2[R:], CANARY)
        out['step'] = dict(param=p2[:R].cpu().numpy(), rss=r2[:R].cpu().numpy(), status=s2[:R].cpu().numpy())
        return out

    def constrained_base(self, which, sigma, other, base, rounds):
        """dc_trace_deconv_ar1_constrained_base, then its last pass alone: dc_trace_deconv_base_step on the state it left."""
        R = self.R
        sigma, other, b = self.vector(sigma), self.vector(other), self.vector(base, True)
        self.outputs()
        state = self.full(7 * R + GUARD)
        param, rss, status = self.full(R + GUARD), self.full(R + GUARD), self.full(R + GUARD, torch.int32)
        self.L.dc_trace_deconv_ar1_constrained_base(self.y, self.f64, self.ld, R, self.T, self.gv, self.gp, self.G, self.ldG, which,
                                                    sigma.data_ptr(), other.data_ptr(), rounds, self.ws.data_ptr(), state.data_ptr(),
                                                    self.c.data_ptr(), self.s.data_ptr(), self.n.data_ptr(), param.data_ptr(), b.data_ptr(),
                                                    rss.data_ptr(), status.data_ptr(), _st())
        out = self.check(param=param, baseline=b, rss=rss, status=status)
        assert _all(state[7 * R:], CANARY)
        p2, b2, r2, s2 = param.clone(), b.clone(), self.full(R + GUARD), self.full(R + GUARD, torch.int32)
        self.L.dc_trace_deconv_base_step(self.y, self.f64, self.ld, R, self.T, self.G, self.ldG, self.ws.data_ptr(), self.n.data_ptr(),
                                         bsref.PASS_LAST, state.data_ptr(), p2.data_ptr(), b2.data_ptr(), r2.data_ptr(), s2.data_ptr(), None,
                                         _st())
        torch.cuda.synchronize()
        assert _all(r2[R:], CANARY) and _all(s2[R:], -7) and _all(p2[R:], CANARY)
        out['step'] = dict(param=p2[:R].cpu().numpy(), rss=r2[:R].cpu().numpy(), status=s2[:R].cpu().numpy())
        return out

    def ar2(self, g1, g2, Hp, ldH, lam, smin, base):
        lam, smin, b = self.vector(lam), self.vector(smin), self.vector(base)
        self.outputs()
        self.L.dc_trace_deconv_ar2(self.y, self.f64, self.ld, self.R, self.T, g1, g2, Hp, ldH, lam.data_ptr(), smin.data_ptr(), b.data_ptr(),
                                   self.ws.data_ptr(), self.c.data_ptr(), self.s.data_ptr(), self.n.data_ptr(), _st())
        return self.check()

    def ar2_constrained(self, g1, g2, Hp, ldH, which, sigma, other, rounds):
        R = self.R
        sigma, other = self.vector(sigma), self.vector(other)
        self.outputs()
        state = self.full(5 * R + GUARD)
        param, rss, status = self.full(R + GUARD), self.full(R + GUARD), self.full(R + GUARD, torch.int32)
        self.L.dc_trace_deconv_ar2_constrained(self.y, self.f64, self.ld, R, self.T, g1, g2, Hp, ldH, which, sigma.data_ptr(), other.data_ptr(),
                                               rounds, self.ws.data_ptr(), state.data_ptr(), self.c.data_ptr(), self.s.data_ptr(),
                                               self.n.data_ptr(), param.data_ptr(), rss.data_ptr(), status.data_ptr(), _st())
        out = self.check(param=param, rss=rss, status=status)
        assert _all(state[5 * R:], CANARY)
        return out


THREE = ('calcium', 'spikes', 'pools')
SEARCH = THREE + ('param', 'rss', 'status')
STEP = ('param', 'rss', 'status')
ROOTS = (GAMMA, math.exp(-1.0 / 1.5))                                    # the decay and the rise of the AR(2) model
ROUNDS = 6


def _bits(got, want, what, names):
    for name in names:
        a, b = np.asarray(got[name]), np.asarray(want[name])
        assert dcref.same_bits(a, b), (what, name, np.argwhere(a != b)[:5].tolist())


def _three(c_s_n):
    return dict(zip(THREE, c_s_n))


def _every_entry_point(dev, y, sigma, gs, ar2_table_ptr=None, ldH=0, what=''):
    """The entry points `dev` can serve against their oracles, in every bit.  gs None: one decay and one table for all traces (then
    also the two AR(2) entry points, whose table is at ar2_table_ptr); otherwise one decay per trace."""
    g = GAMMA if gs is None else gs
    lam, smin, b0 = 0.02, 0.3 * sigma, 0.1 + 0.05 * np.arange(len(y))
    if gs is None:
        _bits(dev.ar1(lam, smin), _three(dcref.deconvolve(y, GAMMA, lam, smin)), what + 'ar1', THREE)
    else:
        want = [dcref.deconvolve(y[r:r + 1], float(gs[r]), lam, smin[r]) for r in range(len(y))]
        _bits(dev.each(lam, smin), _three([np.concatenate([w[i] for w in want]) for i in range(3)]), what + 'each', THREE)
    _bits(dev.base(lam, smin, b0), bsref.deconvolve(y, g, lam, smin, b0, 0), what + 'base', bsref.FIT_NAMES)
    _bits(dev.fit(lam, smin, 0.0, 3), bsref.deconvolve(y, g, lam, smin, 0.0, 3), what + 'fit_base', bsref.FIT_NAMES)
    for which in (srref.SMIN, srref.LAM):
        got = dev.constrained(which, sigma, 0.0, ROUNDS)
        _bits(got, srref.deconvolve(y, g, which, sigma, 0.0, ROUNDS), what + 'constrained %d' % which, SEARCH + ('target',))
        _bits(got['step'], got, what + 'search_step %d' % which, STEP)
    got = dev.constrained_base(srref.SMIN, sigma, 0.0, 0.0, ROUNDS)
    _bits(got, bsref.deconvolve_search(y, g, srref.SMIN, sigma, 0.0, 0.0, ROUNDS), what + 'constrained_base', bsref.SEARCH_NAMES)
    _bits(got['step'], got, what + 'base_step', STEP)
    if ar2_table_ptr is not None:
        g1, g2 = a2ref.coefficients(*ROOTS)
        _bits(dev.ar2(g1, g2, ar2_table_ptr, ldH, lam, smin, b0), _three(a2ref.deconvolve(y, ROOTS[0], ROOTS[1], lam, smin, b0)), what + 'ar2', THREE)
        _bits(dev.ar2_constrained(g1, g2, ar2_table_ptr, ldH, srref.LAM, sigma, 0.0, ROUNDS),
              a2ref.constrained(y, ROOTS[0], ROOTS[1], srref.LAM, sigma, 0.0, ROUNDS), what + 'ar2_constrained', SEARCH)


DECONV = ('dc_trace_deconv_ar1', 'dc_trace_deconv_ar1_each', 'dc_trace_deconv_ar1_base', 'dc_trace_deconv_ar1_fit_base',
          'dc_trace_deconv_ar1_constrained', 'dc_trace_deconv_ar1_constrained_base', 'dc_trace_deconv_search_step',
          'dc_trace_deconv_base_step', 'dc_trace_deconv_ar2', 'dc_trace_deconv_ar2_constrained')


@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('case', ['A', 'B', 'B65'])
def test_deconv_of_rows_beyond_the_line(dclib, case, dtype):
    """The ten entry points read y at stride ld; the tables are small: one for all traces, then one per trace."""
    from deep_calcium_amd.deconv import ar1_table, ar2_table
    case = _row_case(case)
    R, ld, T = case
    with _budget(*DECONV):
        y, sigma, decoy = _traces(case, dtype, 30 + T)
        m = _Rows(case, TORCH_OF[dtype], y, decoy)
        G, Ht = _dev(ar1_table(GAMMA, T)), _dev(ar2_table(ROOTS[0], ROOTS[1], T))
        _every_entry_point(_Deconv(dclib, m.ptr, ld, R, T, dtype == np.float64, G.data_ptr()), y, sigma, None, Ht.data_ptr(), T + 1)
        gs = np.array([GAMMA, math.exp(-1.0 / 2), math.exp(-1.0 / 30)][:R])
        Ge = _dev(np.stack([ar1_table(float(g), T) for g in gs]))
        _every_entry_point(_Deconv(dclib, m.ptr, ld, R, T, dtype == np.float64, Ge.data_ptr(), T + 1, gs), y, sigma, gs, what='each: ')
        m.untouched(y, decoy)


def test_ar1_tables_of_rows_beyond_the_line(dclib):
    """dc_ar1_tables writes two tables at ldG = 2^31 + 8; the eight entry points that take a table per trace then read them there, and
    the two AR(2) entry points read their three-row table at ldH = 2^30 + 5, whose last row starts at 2^31 + 10."""
    from deep_calcium_amd.deconv import ar1_table, ar2_table
    R, ldG, T = wi.ROW_A
    with _budget('dc_ar1_tables'):
        y, sigma, _ = _traces(wi.ROW_A, np.float64, 40)
        dy = _dev(y)
        gs = np.array([math.exp(-1.0 / 2), GAMMA])
        dg = _dev(gs)
        tables = _Rows((R, ldG, T + 1), torch.float64)
        dclib.dc_ar1_tables(dg.data_ptr(), R, T, tables.ptr, ldG, _st())
        tables.written(0, T + 1)
        _same(tables.matrix(), np.stack([ar1_table(float(g), T) for g in gs]), 'tables')
        tables.buf[T + 1:T + 1 + 8] = 0.5                                # the decoy: the T + 1 values at the masked offset 8 are all valid
        _every_entry_point(_Deconv(dclib, dy.data_ptr(), T, R, T, True, tables.ptr, ldG, gs), y, sigma, gs, what='ldG: ')
        del tables
        torch.cuda.empty_cache()
        case = (3, wi.ROW_B[1], T + 1)
        Ht = ar2_table(ROOTS[0], ROOTS[1], T)
        other = ar2_table(math.exp(-1.0 / 20), math.exp(-1.0 / 3), T)
        wide = _Rows(case, torch.float64, Ht, other[2, :wi.decoy_offset(case)])
        dev = _Deconv(dclib, dy.data_ptr(), T, R, T, True, None)
        g1, g2 = a2ref.coefficients(*ROOTS)
        lam, smin, b0 = 0.02, 0.3 * sigma, 0.1 + 0.05 * np.arange(R)
        _bits(dev.ar2(g1, g2, wide.ptr, case[1], lam, smin, b0), _three(a2ref.deconvolve(y, ROOTS[0], ROOTS[1], lam, smin, b0)), 'ldH: ar2', THREE)
        _bits(dev.ar2_constrained(g1, g2, wide.ptr, case[1], srref.LAM, sigma, 0.0, ROUNDS),
              a2ref.constrained(y, ROOTS[0], ROOTS[1], srref.LAM, sigma, 0.0, ROUNDS), 'ldH: ar2_constrained', SEARCH)
        wide.untouched(Ht, None)


# ---- through the Python API: a resident tensor whose row stride is case B's --------------------------------------------------------
def _strided(case, y):
    """(R, T) view of row stride ld into a device buffer of NaN that holds the rows of y, and the decoy behind row 0."""
    R, ld, T = case
    buf = torch.empty((wi.row_elements(case),), dtype=torch.float64, device='cuda')
    buf.fill_(float('nan'))
    view = buf.as_strided((R, T), (ld, 1))
    view.copy_(_dev(y))
    buf[T:T + wi.decoy_offset(case)] = 0.75
    assert view.stride() == (ld, 1) and view[R - 1].data_ptr() - buf.data_ptr() == 8 * wi.last_row_offset(case)
    return buf, view


def test_trace_deconvolver_takes_rows_beyond_the_line():
    from deep_calcium_amd import TraceDeconvolver
    case = wi.ROW_B
    with _budget('dc_trace_deconv_ar1_constrained'):
        y, sigma, _ = _traces(case, np.float64, 50)
        buf, view = _strided(case, y)
        for kw in (dict(s_min=0.1, lam=0.02), dict(constrain='lam', rounds=ROUNDS), dict(constrain='s_min', rounds=ROUNDS, baseline='fit'),
                   dict(s_min=0.1, rise=ROOTS[1])):
            wide, dense = TraceDeconvolver(view, GAMMA, **kw), TraceDeconvolver(_dev(y), GAMMA, **kw)
            kinds = THREE + (('param', 'rss', 'status') if 'constrain' in kw else ())
            for kind in kinds:
                _same(wide.result_device(kind), dense.result_device(kind), (sorted(kw), kind))
            del wide, dense
        del buf, view


def test_ar1_estimator_takes_rows_beyond_the_line():
    from deep_calcium_amd.dynamics import TraceDynamics
    case = wi.ROW_B
    with _budget('dc_trace_ar1_estimate'):
        y, _, _ = _traces(case, np.float64, 51)
        buf, view = _strided(case, y)
        wide, dense = TraceDynamics(view), TraceDynamics(_dev(y))
        for kind in ('noise', 'autocov', 'g_raw'):
            _same(wide.result_device(kind), dense.result_device(kind), kind)
        assert bool(torch.isfinite(wide.result_device('g_raw')).all())
        del wide, dense, buf, view


# =================================================================================================================================
# The accumulators: frames beyond the line (128 x 128, 131113 frames), and sums whose rows lie beyond it
# =================================================================================================================================
def _counts(n):
    """How often each base frame occurs among the n frames of a periodic recording."""
    return np.bincount(gc.rows(n), minlength=K).astype(np.int64)


def _csr_big(rs):
    """Three ROIs on the 128 x 128 frame as CSR rows: two ROIs of their own rows, a third fed by two rows (atomics), pixels from the
    first to the last of the frame.  -> (row_off, row_pix, row_roi, the ROIs' pixel lists)."""
    px = [np.concatenate([[0, 1], rs.choice(H * W, 40, replace=False)]), rs.choice(H * W, 25, replace=False),
          np.concatenate([rs.choice(H * W, 30, replace=False), [H * W - 1]]), rs.choice(H * W, 9, replace=False)]
    off = np.cumsum([0] + [len(p) for p in px])
    roi = [0, 1, 2, 2]
    lists = [px[0], px[1], np.concatenate([px[2], px[3]])]
    return off, np.concatenate(px), roi, lists


@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
def test_roi_sums_of_frames_beyond_the_line(dclib, weighted):
    name = 'dc_roi_wtrace_accumulate' if weighted else 'dc_roi_trace_accumulate'
    dtype = np.uint16 if weighted else np.int16
    t0, pad = 5, 3
    with _budget(name):
        rs = np.random.RandomState(60)
        base = gc.base_frames(rs, (H, W), dtype)
        off, pix, roi, lists = _csr_big(rs)
        wgt = rs.randint(0, 257, size=len(pix)).astype(np.uint16)
        wgt[:2] = [256, 0]
        R, ld = len(lists), t0 + TC + pad
        idx = _idx(TC)
        frames = _periodic(base, idx)
        sums = torch.full((R, ld), GARBAGE, dtype=torch.int64, device='cuda')
        d_off, d_pix, d_roi, d_wgt = _i32(off), _i32(pix), _i32(roi), _dev(wgt)
        if weighted:
            dclib.dc_roi_wtrace_accumulate(frames.data_ptr(), _uns(dtype), TC, t0, d_off.data_ptr(), d_pix.data_ptr(), d_wgt.data_ptr(),
                                           d_roi.data_ptr(), len(off) - 1, R, sums.data_ptr(), ld, H, W, _st())
            want = np.array(wtref.csr_sums(base, off, pix, wgt, roi, R), np.int64)
        else:
            dclib.dc_roi_trace_accumulate(frames.data_ptr(), _uns(dtype), TC, t0, d_off.data_ptr(), d_pix.data_ptr(), d_roi.data_ptr(),
                                          len(off) - 1, R, sums.data_ptr(), ld, H, W, _st())
            want = gc.roi_sums(base, lists)
        torch.cuda.synchronize()
        assert _all(sums[:, :t0], GARBAGE) and _all(sums[:, t0 + TC:], GARBAGE), 'a guard column was written'
        _same(sums[:, t0:t0 + TC].t().contiguous(), _dev(np.ascontiguousarray(want.T))[idx], 'sums')
        del frames, sums


TINY = (2, 3)                         # the frames behind the sums whose rows lie beyond the line
TINY_CSR = {2: ([0, 2, 5, 6], [0, 1, 2, 3, 4, 5], [0, 1, 0], [[0, 1, 5], [2, 3, 4]]),
            3: ([0, 2, 4, 5, 6], [0, 1, 2, 3, 4, 5], [0, 1, 2, 0], [[0, 1, 5], [2, 3], [4]])}


@pytest.mark.parametrize('weighted', [False, True], ids=['plain', 'weighted'])
@pytest.mark.parametrize('case', ROW_IDS)
def test_roi_sums_into_rows_beyond_the_line(dclib, case, weighted):
    """300 frames of 2 x 3 at t0 = 0 into sums of stride ld: the rows fed by atomics are zeroed by the call, at r * ld too."""
    name = 'dc_roi_wtrace_accumulate' if weighted else 'dc_roi_trace_accumulate'
    case = _row_case(case)
    R, ld, T = case
    with _budget(name):
        rs = np.random.RandomState(61)
        frames = _rand(rs, (T,) + TINY, np.int16)
        off, pix, roi, lists = TINY_CSR[R]
        wgt = np.array([256, 0, 17, 255, 1, 128], np.uint16)
        df, d_off, d_pix, d_roi, d_wgt = _dev(frames), _i32(off), _i32(pix), _i32(roi), _dev(wgt)
        sums = _Rows(case, torch.int64)
        if weighted:
            dclib.dc_roi_wtrace_accumulate(df.data_ptr(), 0, T, 0, d_off.data_ptr(), d_pix.data_ptr(), d_wgt.data_ptr(), d_roi.data_ptr(),
                                           len(off) - 1, R, sums.ptr, ld, TINY[0], TINY[1], _st())
            want = np.array(wtref.csr_sums(frames, off, pix, wgt, roi, R), np.int64)
        else:
            dclib.dc_roi_trace_accumulate(df.data_ptr(), 0, T, 0, d_off.data_ptr(), d_pix.data_ptr(), d_roi.data_ptr(), len(off) - 1, R,
                                          sums.ptr, ld, TINY[0], TINY[1], _st())
            want = gc.roi_sums(frames, lists)
        sums.written(0, T)
        _same(sums.matrix(), want, 'sums')


def _pixel_case(rs, shape, n_roi):
    """Entries (CSR rows of support pixels, each row an ROI's) and the ROIs' own pixels on a frame of `shape`."""
    n = shape[0] * shape[1]
    own = [np.sort(rs.choice(n, min(6, n // 2), replace=False)) for _ in range(n_roi)]
    rows = [np.sort(rs.choice(n, min(11, n), replace=False)) for _ in range(n_roi + 1)]          # the last ROI has two rows
    roi = list(range(n_roi)) + [n_roi - 1]
    rows[0][0], rows[-1][-1] = 0, n - 1
    return own, rows, roi


def _pixel_moments(frames, own, rows, roi, weight=None):
    """int64 (4, N), the planes a, b and the two words of c: the sum over the frames (each `weight` times) of the oracle's moments of
    one frame.  -> also the ROIs' traces."""
    weight = np.ones(len(frames), np.int64) if weight is None else weight
    S = [fpref.sums(frames, [int(p) for p in o]) for o in own]
    total = None
    for t in range(len(frames)):
        mom = []
        for p, r in zip(rows, roi):
            mom += fpref.moments(frames[t:t + 1], [int(q) for q in p], S[r][t:t + 1])
        mom = np.array(mom, object) * int(weight[t])
        total = mom if total is None else total + mom
    planes = np.array([[int(a) for a, _, _ in total], [int(b) for _, b, _ in total], [_i64(int(c)) for _, _, c in total],
                       [int(c) >> 64 for _, _, c in total]], np.int64)
    return planes, np.array(S, np.int64)


def test_pixel_moments_of_frames_beyond_the_line(dclib):
    t0, pad = 0, 2
    with _budget('dc_roi_pixel_accumulate'):
        rs = np.random.RandomState(62)
        base = gc.base_frames(rs, (H, W), np.int16)
        own, rows, roi = _pixel_case(rs, (H, W), 2)
        want, S = _pixel_moments(base, own, rows, roi, _counts(TC))
        idx = _idx(TC)
        frames = _periodic(base, idx)
        R, ld = len(own), TC + pad
        sums = torch.full((R, ld), GARBAGE, dtype=torch.int64, device='cuda')
        sums[:, :TC] = _dev(S)[:, idx]
        off = np.cumsum([0] + [len(p) for p in rows])
        N = int(off[-1])
        d_off, d_pix, d_roi = _i32(off), _i32(np.concatenate(rows)), _i32(roi)
        mom = _Out(4 * N, torch.int64)
        mom.buf[mom.lead:mom.lead + 4 * N] = 0
        dclib.dc_roi_pixel_accumulate(frames.data_ptr(), 0, TC, t0, d_off.data_ptr(), d_pix.data_ptr(), d_roi.data_ptr(), len(rows), R,
                                      sums.data_ptr(), ld, mom.ptr, N, H, W, _st())
        _same(mom.get(4, N), want, 'moments')
        del frames, sums


@pytest.mark.parametrize('case', ROW_IDS)
def test_pixel_moments_from_rows_beyond_the_line(dclib, case):
    """The ROI traces the pixel moments are taken against lie at stride ld: the last ROI's beyond the line."""
    case = _row_case(case)
    R, ld, T = case
    with _budget('dc_roi_pixel_accumulate'):
        rs = np.random.RandomState(63)
        frames = _rand(rs, (T,) + TINY, np.int16)
        own, rows, roi = _pixel_case(rs, TINY, R)
        want, S = _pixel_moments(frames, own, rows, roi)
        decoy = rs.randint(-1000, 1000, size=wi.decoy_offset(case)).astype(np.int64)
        sums = _Rows(case, torch.int64, S, decoy)
        off = np.cumsum([0] + [len(p) for p in rows])
        N = int(off[-1])
        df, d_off, d_pix, d_roi = _dev(frames), _i32(off), _i32(np.concatenate(rows)), _i32(roi)
        mom = _Out(4 * N, torch.int64)
        mom.buf[mom.lead:mom.lead + 4 * N] = 0
        dclib.dc_roi_pixel_accumulate(df.data_ptr(), 0, T, 0, d_off.data_ptr(), d_pix.data_ptr(), d_roi.data_ptr(), len(rows), R, sums.ptr, ld,
                                      mom.ptr, N, TINY[0], TINY[1], _st())
        _same(mom.get(4, N), want, 'moments')
        sums.untouched(S, decoy)


def test_pair_sums_of_frames_beyond_the_line(dclib):
    """a = sum x and g = sum x x' over the pixels of two ROIs, one of 70 pixels (two tiles of 64), summed over all frames."""
    with _budget('dc_roi_pair_accumulate'):
        rs = np.random.RandomState(64)
        base = gc.base_frames(rs, (H, W), np.uint16)
        flats = [np.concatenate([[0], rs.choice(np.arange(1, H * W - 1), 68, replace=False), [H * W - 1]]), rs.choice(H * W, 5, replace=False)]
        roi_off, goff, tiles, G = paref.layout([len(f) for f in flats])
        P, cnt = roi_off[-1], _counts(TC)
        want_a, want_g = np.zeros(P, object), np.zeros(G, object)
        for k in range(K):
            for r, flat in enumerate(flats):
                a, g = paref.moments(base[k:k + 1], [int(p) for p in flat])
                n = len(flat)
                want_a[roi_off[r]:roi_off[r] + n] += int(cnt[k]) * np.array(a, object)
                for i in range(n):
                    for j in range(i, n):                                # the upper triangle of the tiles ti <= tj is what is accumulated
                        want_g[goff[r] + i * n + j] += int(cnt[k]) * g[i][j]
        idx = _idx(TC)
        frames = _periodic(base, idx)
        d_off, d_pix, d_goff, d_tiles = _i32(roi_off), _i32(np.concatenate(flats)), _dev(np.array(goff, np.int64)), _i32(tiles)
        a, g = _Out(P, torch.int64), _Out(G, torch.int64)
        a.buf[a.lead:a.lead + P] = 0
        g.buf[g.lead:g.lead + G] = 0
        dclib.dc_roi_pair_accumulate(frames.data_ptr(), 1, TC, d_off.data_ptr(), d_pix.data_ptr(), d_goff.data_ptr(), d_tiles.data_ptr(),
                                     len(tiles), len(flats), a.ptr, g.ptr, P, G, H, W, _st())
        _same(a.get(P), want_a.astype(np.int64), 'a')
        got_g = g.get(G).cpu().numpy()
        for r, flat in enumerate(flats):                                 # compared where the header says a word is written: see below
            n = len(flat)
            gg, ww = got_g[goff[r]:goff[r] + n * n].reshape(n, n), want_g[goff[r]:goff[r] + n * n].reshape(n, n).astype(np.int64)
            upper = np.triu(np.ones((n, n), bool))
            assert np.array_equal(gg[upper], ww[upper]), ('g', r)
        del frames


# =================================================================================================================================
# The frame route: csrc/motion.hip, csrc/series.hip, csrc/frame_quality.hip
# =================================================================================================================================
@pytest.mark.parametrize('dtype', [np.int16, np.uint16], ids=['int16', 'uint16'])
def test_scores_of_frames_beyond_the_line(dclib, dtype):
    S = 1
    with _budget('dc_motion_ssd'):
        rs = np.random.RandomState(70)
        base, tmpl = gc.base_frames(rs, (H, W), dtype), _rand(rs, (H, W), dtype)
        idx = _idx(TC)
        frames, dt = _periodic(base, idx), _dev(tmpl)
        nd = 2 * S + 1
        out = _Out(TC * nd * nd, torch.int64)
        dclib.dc_motion_ssd(frames.data_ptr(), _uns(dtype), TC, dt.data_ptr(), H, W, S, out.ptr, _st())
        _same(out.get(TC, nd, nd), _dev(ref.scores(base, tmpl, S))[idx], 'scores')
        del frames


def _centre_rows(rs, lim):
    named = [(0, 0), (1, -1), (-1, 1), (1, 1), (-1, -1), (2, 0), (-1, 0), (0, -2), (0, 1), (-5, 7), (I32_MAX, -I32_MAX),
             (-2 ** 31, I32_MAX), (0, -2 ** 31)]
    more = [tuple(int(v) for v in rs.randint(-lim, lim + 1, size=2)) for _ in range(K - len(named))]
    return np.array(named + more, np.int64)


def test_window_scores_of_frames_beyond_the_line(dclib):
    S, D, mult, dtype = 3, 1, 2, np.uint16
    with _budget('dc_motion_ssd_around'):
        rs = np.random.RandomState(71)
        base, tmpl, rows = gc.base_frames(rs, (H, W), dtype), _rand(rs, (H, W), dtype), _centre_rows(rs, 3)
        idx = _idx(TC)
        frames, dt, dr = _periodic(base, idx), _dev(tmpl), _periodic(rows.astype(np.int32), idx)
        nd = 2 * D + 1
        out = _Out(TC * nd * nd, torch.int64)
        dclib.dc_motion_ssd_around(frames.data_ptr(), _uns(dtype), TC, dt.data_ptr(), H, W, S, D, dr.data_ptr(), mult, out.ptr, _st())
        _same(out.get(TC, nd, nd), _dev(wref.window_scores(base, tmpl, S, D, rows, mult))[idx], 'window scores')
        del frames


def test_block_scores_of_frames_beyond_the_line(dclib):
    S, D, By, Bx, dtype = 1, 1, 2, 2, np.int16
    with _budget('dc_motion_block_ssd'):
        rs = np.random.RandomState(72)
        base, tmpl = gc.base_frames(rs, (H, W), dtype), _rand(rs, (H, W), dtype)
        rigid = rs.randint(-S - 2, S + 3, size=(K, 2)).astype(np.int64)
        rigid[:3] = [(1000, -1000), (-2 ** 31, I32_MAX), (S, -S)]
        idx = _idx(TC)
        frames, dt, dr = _periodic(base, idx), _dev(tmpl), _periodic(rigid.astype(np.int32), idx)
        nd = 2 * D + 1
        out = _Out(TC * By * Bx * nd * nd, torch.int64)
        dclib.dc_motion_block_ssd(frames.data_ptr(), _uns(dtype), TC, dt.data_ptr(), H, W, S, D, By, Bx, dr.data_ptr(), out.ptr, _st())
        _same(out.get(TC, By, Bx, nd, nd), _dev(bref.block_scores(base, tmpl, S, D, By, Bx, rigid))[idx], 'block scores')
        del frames


def _shifts(rs, fine):
    """K shifts (whole pixels, or sixteenths): inside, on the edge of and beyond the frame, the int32 extremes, random ones."""
    q = 16 if fine else 1
    named = [(0, 0), (q, -q), (-q, q), (q * (H - 1), q * (W - 1)), (q * (1 - H), q * (1 - W)), (q * H, 0), (0, -q * W), (I32_MAX, 0),
             (0, -2 ** 31), (-2 ** 31, I32_MAX)]
    if fine:
        named += [(1, -1), (15, -15), (17, -17), (37, 0), (0, 37), (-40, 23), (8, 8)]
    more = [(int(rs.randint(-q * 6, q * 6 + 1)), int(rs.randint(-q * 6, q * 6 + 1))) for _ in range(K - len(named))]
    return np.array(named + more, np.int64)


def _block_shifts(rs, By, Bx, fine):
    q = 16 if fine else 1
    bs = rs.randint(-3 * q, 3 * q + 1, size=(K, By, Bx, 2)).astype(np.int64)
    bs[1] = (q * H, 0)                                                   # all fill
    bs[2, :, 1] = (0, -q * W)                                            # the middle column of blocks leaves the frame
    bs[3] = 0
    bs[4, 0, 0] = (I32_MAX, -2 ** 31)
    return bs


def _mover(dclib, name, rs):
    """-> (the base frames, launch(frames pointer, idx, out pointer) -> the table it must keep alive, the oracle's result on the base)."""
    By, Bx = 2, 3
    if name == 'dc_bidi_apply':
        base = gc.base_frames(rs, (H, W), np.int16)
        return base, (lambda f, idx, o: dclib.dc_bidi_apply(f, TC, 3, H, W, 7, o, _st())), biref.apply(base, 3, 7)
    fine, blocks = name.endswith('_sub'), 'warp' in name
    dtype, fill = (np.uint16, 48879) if name == 'dc_motion_apply_sub' else (np.int16, -2)
    base = gc.base_frames(rs, (H, W), dtype)
    table = _block_shifts(rs, By, Bx, fine) if blocks else _shifts(rs, fine)
    oracle = {'dc_motion_apply': ref.apply, 'dc_motion_apply_sub': sref.apply_sub, 'dc_motion_warp': bref.warp, 'dc_motion_warp_sub': sref.warp_sub}

    def launch(f, idx, o):
        t = _periodic(table.astype(np.int32), idx)
        if name == 'dc_motion_apply':
            dclib.dc_motion_apply(f, TC, t.data_ptr(), H, W, fill, o, _st())
        elif name == 'dc_motion_apply_sub':
            dclib.dc_motion_apply_sub(f, _uns(dtype), TC, t.data_ptr(), H, W, fill, o, _st())
        elif name == 'dc_motion_warp':
            dclib.dc_motion_warp(f, TC, t.data_ptr(), By, Bx, H, W, fill, o, _st())
        else:
            dclib.dc_motion_warp_sub(f, _uns(dtype), TC, t.data_ptr(), By, Bx, H, W, fill, o, _st())
        return t
    return base, launch, oracle[name](base, table, fill)


@pytest.mark.parametrize('name', ['dc_motion_apply', 'dc_motion_apply_sub', 'dc_motion_warp', 'dc_motion_warp_sub', 'dc_bidi_apply'])
def test_moved_frames_beyond_the_line(dclib, name):
    """frames and out both pass 2^31 values; out starts 3 values into its allocation: no frame of it starts on a group of 8."""
    with _budget(name):
        rs = np.random.RandomState(80)
        base, launch, want = _mover(dclib, name, rs)
        assert want.shape == base.shape and want.dtype == base.dtype and (want != base).any()
        idx = _idx(TC)
        frames = _periodic(base, idx)
        out = _Out(TC * H * W, torch.int16, odd=3)
        keep = launch(frames.data_ptr(), idx, out.ptr)
        got = out.get(TC, H, W)
        del frames, keep
        _same(got, _dev(want)[idx], 'moved frames')
        del got, out


def test_bidi_scores_of_frames_beyond_the_line(dclib):
    P, dtype = 2, np.uint16
    with _budget('dc_bidi_scores'):
        rs = np.random.RandomState(81)
        base = gc.base_frames(rs, (H, W), dtype)
        idx = _idx(TC)
        frames = _periodic(base, idx)
        nd = 2 * P + 1
        out = _Out(TC * nd, torch.int64)
        dclib.dc_bidi_scores(frames.data_ptr(), _uns(dtype), TC, H, W, P, out.ptr, _st())
        _same(out.get(TC, nd), _dev(np.asarray(biref.scores(base, P), np.int64))[idx], 'scores')
        del frames


@pytest.mark.parametrize('dtype', [np.int16, np.uint16], ids=['int16', 'uint16'])
def test_series_sums_of_frames_beyond_the_line(dclib, dtype):
    """sum, sumsq, vmax and the four cross sums of the whole recording in one chunk: each base frame's share, times how often it occurs."""
    with _budget('dc_series_accumulate', 'dc_series_accumulate_xy'):
        rs = np.random.RandomState(82)
        base = gc.base_frames(rs, (H, W), dtype)
        x, cnt = base.astype(np.int64), _counts(TC)
        want = dict(sum=np.tensordot(cnt, x, 1), sumsq=np.tensordot(cnt, x * x, 1), vmax=x.max(0).astype(np.int32),
                    xy=sum(int(cnt[k]) * _xy_ref(x[k:k + 1]) for k in range(K)))
        assert len(set(cnt.tolist())) == 2                               # a frame read twice, or another one in its place, changes a sum
        frames = _periodic(base, _idx(TC))
        n = H * W
        s1, s2, vm, xy = _Out(n, torch.int64), _Out(n, torch.int64), _Out(n, torch.int32), _Out(4 * n, torch.int64)
        dclib.dc_series_accumulate(frames.data_ptr(), _uns(dtype), TC, 0, TC, None, None, s1.ptr, s2.ptr, vm.ptr, H, W, _st())
        dclib.dc_series_accumulate_xy(frames.data_ptr(), _uns(dtype), TC, 0, xy.ptr, H, W, _st())
        _same(s1.get(H, W), want['sum'], 'sum')
        _same(s2.get(H, W), want['sumsq'], 'sumsq')
        _same(vm.get(H, W), want['vmax'], 'vmax')
        _same(xy.get(4, H, W), want['xy'], 'xy')
        del frames


def test_time_bins_of_frames_beyond_the_line(dclib):
    """b = 2 from phase 0: bin i holds frames 2 i and 2 i + 1, so the bins have period 37 as well; the last frame stays in carry."""
    b, dtype = 2, np.int16
    with _budget('dc_series_bin_time'):
        rs = np.random.RandomState(83)
        base = gc.base_frames(rs, (H, W), dtype)
        bins = tbref.bin_time(gc.expand(base, 2 * K), b)                 # bin i of these 37 is every bin i + 37 j of the recording
        n_out = TC // b
        assert TC % b == 1 and bins.shape[0] == K and 2 * (n_out - 1) * H * W > wi.LINE
        frames = _periodic(base, _idx(TC))
        out, carry = _Out(n_out * H * W, torch.int16, odd=3), _Out(H * W, torch.int32)
        dclib.dc_series_bin_time(frames.data_ptr(), _uns(dtype), TC, H, W, b, 0, carry.ptr, out.ptr, _st())
        got = out.get(n_out, H, W)
        _same(carry.get(H, W), base[(TC - 1) % K].astype(np.int32), 'carry')
        del frames
        _same(got, _dev(bins)[_idx(n_out)], 'bins')
        del got, out


def test_frame_moments_beyond_the_line(dclib):
    """(sum x, sum x^2, sum x tmpl) per frame over a rectangle that leaves out a row and a column on every side."""
    dtype, rect = np.uint16, ((1, H - 1), (1, W - 1))
    with _budget('dc_frame_moments'):
        rs = np.random.RandomState(84)
        base, tmpl = gc.base_frames(rs, (H, W), dtype), _rand(rs, (H, W), dtype)
        idx = _idx(TC)
        frames, dt = _periodic(base, idx), _dev(tmpl)
        mom = _Out(3 * TC, torch.int64)
        dclib.dc_frame_moments(frames.data_ptr(), _uns(dtype), TC, dt.data_ptr(), H, W, rect[0][0], rect[0][1], rect[1][0], rect[1][1], mom.ptr, _st())
        _same(mom.get(TC, 3), _dev(np.array(frref.moments_np(base, tmpl, rect), np.int64))[idx], 'moments')
        del frames


def test_gathered_frames_beyond_the_line(dclib):
    """k = 131113 indices that jump between both sides of frame 131072, two of them outside the recording: `out` passes 2^31 values
    too, and starts 3 values into its allocation."""
    dtype = np.int16
    with _budget('dc_frame_gather'):
        rs = np.random.RandomState(85)
        base = gc.base_frames(rs, (H, W), dtype)
        k = TC
        pick = (torch.arange(k, device='cuda') * 7919) % TC              # 7919 is prime to 131113 = 7 x 18730 + 3: a permutation
        pick[5], pick[k - 1] = -1, TC
        assert int((pick >= 131072).sum()) == 41 + 1 and int(pick[1]) == 7919       # 41 frames beyond the line, among the others
        table = frref.gather(base, [-1] + list(range(K)))                # entry 0: the frame of an index outside the recording
        code = torch.where((pick >= 0) & (pick < TC), pick % K + 1, torch.zeros_like(pick))
        frames, ix = _periodic(base, _idx(TC)), pick.to(torch.int32)
        out = _Out(k * H * W, torch.int16, odd=3)
        dclib.dc_frame_gather(frames.data_ptr(), TC, ix.data_ptr(), k, H, W, out.ptr, _st())
        got = out.get(k, H, W)
        del frames
        _same(got, _dev(table)[code], 'gathered frames')
        del got, out


# =================================================================================================================================
# The two capped grids DESIGN.md 4f-caps left open: 2^20 workgroups of 256 items
# =================================================================================================================================
def test_binned_frames_beyond_the_cap_and_the_line(dclib):
    """c = 2 on 2^18 + 41 frames of 128 x 128: 1024 items per frame, so item 2^28, the first of frame 2^18, is the first of the second
    trip, and the frames pass 2^31 values from frame 2^17 on: the cap case is the line case of `frames`.  `out` holds 2^30 + 167936
    values: 2 GiB, its byte offsets pass 2^31, its element offsets do not (that needs 16 GiB of frames beside 8 GiB of results)."""
    c, dtype, tc = wi.BIN_C, np.uint16, wi.CAP_TC
    with _budget('dc_motion_bin'):
        rs = np.random.RandomState(90)
        base = gc.base_frames(rs, (H, W), dtype)
        idx = _idx(tc)
        frames = _periodic(base, idx)
        Hc, Wc = H // c, W // c
        out = _Out(tc * Hc * Wc, torch.int16, odd=3)
        dclib.dc_motion_bin(frames.data_ptr(), _uns(dtype), tc, H, W, c, out.ptr, _st())
        got = out.get(tc, Hc, Wc)
        del frames
        _same(got, _dev(wref.bin_frames(base, c))[idx], 'binned frames')
        del got, out


def test_block_refine_of_items_beyond_the_cap(dclib):
    """32 x 32 blocks, D = 0, S = 1, 2^18 + 41 frames: 2^28 + 41984 items, the last 41984 on a second trip; bscores, block_shifts and
    fine are 2 GiB each, 2 it + 1 passes 2^29.  D = 0 leaves the refinement no neighbour (test_motion_sub_gpu.py pins that
    arithmetic at D >= 1): what is pinned here is which item, which frame's rigid shift and which table a thread takes."""
    (By, Bx), S, D, tc = wi.REFINE_BLOCKS, 1, 0, wi.CAP_TC
    with _budget('dc_motion_block_refine'):
        rs = np.random.RandomState(91)
        rigid = rs.randint(-S - 2, S + 3, size=(K, 2)).astype(np.int64)
        rigid[:4] = [(77, -5), (-2 ** 31, I32_MAX), (S, -S), (0, 0)]
        bs = rs.randint(-S - 1, S + 2, size=(K, By, Bx, 2)).astype(np.int64)
        bs[0, 0, 0], bs[1, -1, -1] = (I32_MAX // 16, -(2 ** 31 // 16)), (5, -5)
        bsc = rs.randint(0, 2 ** 62, size=(K, By, Bx, 1, 1)).astype(np.int64)
        want = sref.block_refine(bsc, rigid, bs, S)
        assert want.shape == (K, By, Bx, 2) and len({a.tobytes() for a in want}) == K
        idx = _idx(tc)
        d_sc, d_r, d_bs = _periodic(bsc, idx), _periodic(rigid.astype(np.int32), idx), _periodic(bs.astype(np.int32), idx)
        fine = _Out(tc * By * Bx * 2, torch.int32)
        dclib.dc_motion_block_refine(d_sc.data_ptr(), d_r.data_ptr(), d_bs.data_ptr(), tc, By, Bx, S, D, fine.ptr, _st())
        got = fine.get(tc, By, Bx, 2)
        del d_sc, d_bs
        _same(got, _dev(np.asarray(want).astype(np.int32))[idx], 'fine')
        del got, fine
