"""dF/F traces on the device (include/dcunet.h dc_trace_combine / dc_trace_baseline / dc_trace_scale; deep_calcium_amd/dff.py)
against tests/_dff_ref.py: plain numpy int64, np.sort(window)[k] per frame, a brute-force ring.  Everything is compared exactly:
the integers as integers, the floats bit for bit.

The baseline kernel gives one workgroup a tile of 256 output frames (kTile in csrc/dff.hip): T = 255, 256, 257 and 3 * 256 + 17
sit on either side of one and of several tile boundaries, and a half-width of 300 makes a window reach into two neighbours."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _dff_ref as ref      # noqa: E402

TILE = 256
GARBAGE = -0x0123456789abcdef
GUARD = 6
LIM = 2 ** 62 - 1


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _padded(num, pad):
    """(R, T) -> a device matrix of row stride T + pad with garbage between the rows, and the view of its first T columns."""
    R, T = num.shape
    buf = np.full((R, T + pad), GARBAGE, np.int64)
    buf[:, :T] = num
    return torch.from_numpy(buf).cuda()


class _Out(object):
    """A dense [R][T] output inside a garbage-prefilled buffer with guard elements on both sides: only [R][T] may change."""

    def __init__(self, R, T, dtype):
        self.n = R * T
        self.fill = GARBAGE if dtype == torch.int64 else -7.25
        self.buf = torch.full((self.n + 2 * GUARD,), self.fill, dtype=dtype, device='cuda')
        self.ptr = self.buf.data_ptr() + GUARD * self.buf.element_size()
        self.shape = (R, T)

    def get(self):
        a = self.buf.cpu().numpy()
        assert (a[:GUARD] == self.fill).all() and (a[GUARD + self.n:] == self.fill).all(), 'a guard element was written'
        return a[GUARD:GUARD + self.n].reshape(self.shape).copy()


def _baseline(L, num, half, q, pad=5, base=True, dff=True):
    R, T = num.shape
    d = _padded(num, pad)
    ob, od = _Out(R, T, torch.int64), _Out(R, T, torch.float32)
    L.dc_trace_baseline(d.data_ptr(), T + pad, R, T, half, q, ob.ptr if base else None, od.ptr if dff else None,
                        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    back = d.cpu().numpy()
    assert np.array_equal(back[:, :T], num) and (back[:, T:] == GARBAGE).all()          # the input is only read
    gb, gd = ob.get(), od.get()
    if not base:
        assert (gb == GARBAGE).all()
    if not dff:
        assert (gd == np.float32(-7.25)).all()
    return gb, gd


def _check(L, num, half, q, tag=None, **kw):
    want_b = ref.baseline(num, half, q)
    got_b, got_d = _baseline(L, num, half, q, **kw)
    assert np.array_equal(got_b, want_b), (tag, half, q)
    assert np.array_equal(_bits(got_d), _bits(ref.dff(num, want_b))), (tag, half, q)
    return got_b, got_d


HALVES = (0, 1, 7, 128, 300)
QS = (0, 1, 8, 29, 50, 99, 100)


# ---- 1. dc_trace_baseline ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 2, 5, 255, 256, 257, 3 * TILE + 17])
def test_baseline_equals_the_sorted_window_for_every_length_window_and_percentile(dclib, T):
    rs = np.random.RandomState(T)
    for R in (1, 3):
        num = rs.randint(1000, 5001, size=(R, T)).astype(np.int64)
        for half in HALVES:                       # half >= T: every window is the whole trace
            for q in QS:
                _check(dclib, num, half, q, tag=(T, R))


def test_baseline_of_many_rois(dclib):
    rs = np.random.RandomState(300)
    num = rs.randint(1000, 5001, size=(300, 64)).astype(np.int64)
    for half, q in ((7, 8), (128, 50)):
        _check(dclib, num, half, q, pad=0)


def test_baseline_at_the_maximum_window(dclib):
    rs = np.random.RandomState(2047)
    num = rs.randint(1000, 5001, size=(2, 4200)).astype(np.int64)
    num[1] += (np.arange(4200) * 3) % 1711        # a drifting row
    for q in (8, 100):
        _check(dclib, num, 2047, q)


def _special_traces(T):
    rs = np.random.RandomState(5)
    rows = {
        'random': rs.randint(1000, 5001, size=T),
        'constant': np.full(T, 4242),
        'two-valued': np.where(rs.rand(T) < 0.5, 1000, 1001),                 # heavy in ties
        'ramp': np.arange(T),
        'extremes': np.where(rs.rand(T) < 0.5, -LIM, LIM),                    # hi - lo = 2^63 - 2: the midpoint-overflow case
        'extremes and between': np.concatenate([[-LIM, LIM], rs.randint(-2 ** 40, 2 ** 40, size=T - 2)]),
        'non-positive': -rs.randint(0, 5000, size=T),                         # B <= 0 everywhere: dff is exactly 0
        'crossing zero': rs.randint(-3000, 3001, size=T),
    }
    return list(rows), np.stack([np.asarray(v, np.int64) for v in rows.values()])


def test_baseline_of_ties_ramps_extremes_and_signs(dclib):
    T = 3 * TILE + 17
    names, num = _special_traces(T)
    assert num[names.index('extremes')].min() == -LIM and num[names.index('extremes')].max() == LIM
    for half in (1, 7, 300):
        for q in (0, 8, 29, 50, 100):
            b, d = _check(dclib, num, half, q, tag='special')
            k = ref.rank(q, 2 * half + 1)
            r = names.index('ramp')
            t = np.arange(half, T - half)
            assert np.array_equal(b[r, half:T - half], t - half + k)          # the interior of a ramp
            assert np.array_equal(b[names.index('constant')], np.full(T, 4242)) and (d[names.index('constant')] == 0).all()
            r = names.index('non-positive')
            assert (b[r] <= 0).all() and (_bits(d[r]) == 0).all()             # +0.0, not -0.0 and not a division
            r = names.index('crossing zero')
            assert (_bits(d[r][b[r] <= 0]) == 0).all()
            if q <= 29:                                                       # a low rank of values around zero: negative somewhere
                assert (b[r] <= 0).any()
            if q == 100:
                assert (b[r] > 0).any() and (d[r][b[r] > 0] <= 0).all()         # under its maximum a trace never rises
    # a row that is 0 throughout divides nothing
    b, d = _check(dclib, np.zeros((1, 40), np.int64), 3, 50)
    assert (b == 0).all() and (_bits(d) == 0).all()


def test_each_output_alone_gives_the_same_bits(dclib):
    T = TILE + 41
    _, num = _special_traces(T)
    for half, q in ((0, 8), (7, 29), (128, 8)):
        both_b, both_d = _check(dclib, num, half, q)
        only_b, _ = _baseline(dclib, num, half, q, dff=False)
        _, only_d = _baseline(dclib, num, half, q, base=False)
        assert np.array_equal(only_b, both_b) and np.array_equal(_bits(only_d), _bits(both_d))
    # neither output, no rows, no frames: nothing is launched, nothing is written
    _baseline(dclib, num, 7, 8, base=False, dff=False)
    p = torch.zeros(8, dtype=torch.int64, device='cuda').data_ptr()
    assert dclib.dc_trace_baseline(p, 8, 0, 8, 3, 8, p, p, None) == 0 and dclib.dc_trace_baseline(p, 8, 1, 0, 3, 8, p, p, None) == 0


def test_a_window_of_one_frame_is_the_trace_itself(dclib):
    _, num = _special_traces(TILE + 3)
    for q in (0, 8, 100):
        b, d = _check(dclib, num, 0, q)
        assert np.array_equal(b, num) and (_bits(d) == 0).all()               # num > 0: (N - N) / N; elsewhere 0 by definition


# ---- 2. dc_trace_combine, dc_trace_scale ----------------------------------------------------------------------------------------------
def test_combine_is_int64_arithmetic_on_any_row(dclib):
    rs = np.random.RandomState(9)
    for R, extra, T, pad in ((1, 0, 1, 0), (3, 2, 5, 3), (7, 7, TILE + 1, 1), (5, 0, 3 * TILE + 17, 4), (300, 40, 64, 0)):
        rows = R + extra
        sums = rs.randint(-2 ** 30, 2 ** 30, size=(rows, T)).astype(np.int64)
        ca = rs.randint(-2 ** 30, 2 ** 30, size=R).astype(np.int64)          # |ca S|, |cb Sn| < 2^60, |cc| < 2^60: no overflow
        cb = rs.randint(-2 ** 30, 2 ** 30, size=R).astype(np.int64)
        cc = rs.randint(-2 ** 60, 2 ** 60, size=R).astype(np.int64)
        np_row = rs.randint(0, rows, size=R).astype(np.int32)                 # any row: an ROI's, its own, or one >= R
        np_row[::3] = -1 - rs.randint(0, 5, size=len(np_row[::3]))            # no second term
        if extra:
            np_row[-1] = rows - 1
            assert (np_row >= R).any()
        want = ca[:, None] * sums[:R] + cc[:, None]
        for r in range(R):
            if np_row[r] >= 0:
                want[r] -= cb[r] * sums[np_row[r]]
        d = _padded(sums, pad)
        out = _Out(R, T, torch.int64)
        dev = [torch.from_numpy(a).cuda() for a in (np_row, ca, cb, cc)]
        dclib.dc_trace_combine(d.data_ptr(), T + pad, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), R, T,
                               out.ptr, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(out.get(), want), (R, T)
        assert np.array_equal(d.cpu().numpy()[:, :T], sums)


def test_scale_is_numpys_float64_divide_and_zero_without_a_denominator(dclib):
    rs = np.random.RandomState(10)
    for R, T, pad in ((1, 1, 0), (4, 5, 3), (6, TILE + 1, 1), (300, 64, 0)):
        x = rs.randint(-2 ** 61, 2 ** 61, size=(R, T)).astype(np.int64)
        x[0, 0] = LIM
        den = rs.randint(1, 2 ** 45, size=R).astype(np.int64)
        den[1::4] = 0
        den[2::4] = -rs.randint(1, 2 ** 45, size=len(den[2::4]))
        if R > 3:
            den[3] = 3
        d, dd = _padded(x, pad), torch.from_numpy(den).cuda()
        out = _Out(R, T, torch.float32)
        dclib.dc_trace_scale(d.data_ptr(), T + pad, dd.data_ptr(), R, T, out.ptr, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = out.get()
        assert np.array_equal(_bits(got), _bits(ref.scale(x, den))), (R, T)
        assert (_bits(got[den <= 0]) == 0).all()


# ---- 3. the product path ----------------------------------------------------------------------------------------------------------
T0, H0, W0 = 97, 24, 20
WINDOW, Q = 31, 8


def _recording(dtype, seed=0):
    """(97, 24, 20): a drifting background and three neurons with transients, one of them in the image's corner."""
    rs = np.random.RandomState(seed)
    raw = rs.randint(200, 400, size=(T0, H0, W0)) + (np.arange(T0) * 2)[:, None, None]
    rois = [np.argwhere(np.ones((3, 3))) + [4, 4], np.argwhere(np.ones((2, 4))) + [15, 10], np.array([[23, 19], [22, 19]])]
    for i, c in enumerate(rois):
        raw[:, c[:, 0], c[:, 1]] += ((rs.rand(T0) < 0.1) * rs.randint(500, 3000, size=T0))[:, None] * (i + 1)
    if dtype == np.int16:
        raw = raw - 1500                          # negative sums
    return raw.astype(dtype), [np.asarray(c, np.int64) for c in rois]


def _sums(raw, coords):
    x = raw.astype(np.int64)
    return np.stack([x[:, c[:, 0], c[:, 1]].sum(1) if len(c) else np.zeros(len(x), np.int64) for c in coords])


def _oracle(raw, rois, neuropil=None, offset=0):
    S, A = _sums(raw, rois), np.array([len(c) for c in rois], np.int64)
    if neuropil is None:
        N, D = ref.numerators(S, A, offset=offset)
    else:
        rings = ref.rings(rois, raw.shape[1:], neuropil[0], neuropil[1])
        N, D = ref.numerators(S, A, _sums(raw, rings), np.array([len(c) for c in rings]), neuropil[2], offset)
    B = ref.baseline(N, WINDOW // 2, Q)
    return {'num': N, 'baseline_sum': B, 'f': ref.scale(N, D), 'baseline': ref.scale(B, D), 'dff': ref.dff(N, B)}, D


def _same(got, want, tag):
    assert got.dtype == want.dtype and got.shape == want.shape, tag
    if want.dtype == np.float32:
        assert np.array_equal(_bits(got), _bits(want)), tag
    else:
        assert np.array_equal(got, want), tag


@pytest.mark.parametrize('dtype', [np.int16, np.uint16], ids=['int16', 'uint16'])
def test_every_kind_is_the_oracle_for_every_chunking(tmp_path, dtype):
    from deep_calcium_amd import RoiTraceExtractor, TraceBaseline, dff_traces_device
    from deep_calcium_amd.dff import KINDS
    raw, rois = _recording(dtype)
    path = str(tmp_path / 'rec.npz')
    np.savez(path, series_raw=raw)
    neuropil = (1, 4, 0.7)
    for np_arg, offset in ((None, 0), (neuropil, 0), (neuropil, 1600)):
        want, D = _oracle(raw, rois, np_arg, offset)
        for chunk in (1, 7, T0):
            for kind in KINDS:
                got = dff_traces_device(path, rois, WINDOW, percentile=Q, kind=kind, neuropil=np_arg, offset=offset, chunk_frames=chunk)
                _same(got, want[kind], (np_arg, offset, chunk, kind))
    # the same through TraceBaseline: numpy sums, and the extractor's own sums read in place on the device
    S, A = _sums(raw, rois), [len(c) for c in rois]
    rings = ref.rings(rois, (H0, W0), 1, 4)
    Sn, An = _sums(raw, rings), [len(c) for c in rings]
    want, D = _oracle(raw, rois, neuropil, 1600)
    ext = RoiTraceExtractor((H0, W0), T0, dtype, rois + [c for c in rings if len(c)], chunk_frames=7)
    for a in range(0, T0, 7):
        ext.feed(raw[a:a + 7])
    assert ext.areas_host().tolist() == A + [n for n in An if n] and ext.areas_host().dtype == np.int32
    dev = ext.sums_device()
    assert dev.is_cuda and dev.data_ptr() == ext.sums.data_ptr() and np.array_equal(dev[:len(rois)].cpu().numpy(), S)
    for sums, nsums in ((S, Sn), (dev[:len(rois)], torch.from_numpy(Sn).cuda()), (S, torch.from_numpy(Sn).cuda())):
        tb = TraceBaseline(sums, A, WINDOW, percentile=Q, offset=1600, neuropil_sums=nsums, neuropil_areas=An, weight=0.7)
        assert np.array_equal(tb.denominators(), D) and tb.denominators().dtype == np.int64
        for kind in KINDS:
            _same(tb.result(kind), want[kind], kind)
    tb = TraceBaseline(dev[:len(rois)], A, WINDOW, percentile=Q)
    want, D = _oracle(raw, rois)
    for kind in KINDS:
        _same(tb.result(kind), want[kind], kind)
    assert np.array_equal(tb.denominators(), A)


def test_known_shifts_are_passed_through_to_the_extractor(tmp_path):
    from deep_calcium_amd import dff_traces_device, extract_traces_device
    raw, rois = _recording(np.int16, seed=1)
    path = str(tmp_path / 'rec.npz')
    np.savez(path, series_raw=raw)
    rs = np.random.RandomState(6)
    plain = extract_traces_device(path, rois, kind='sum')
    for name, table in (('shifts', rs.randint(-3, 4, size=(T0, 2))), ('fine_shifts', rs.randint(-40, 41, size=(T0, 2)))):
        moved = extract_traces_device(path, rois, kind='sum', chunk_frames=16, **{name: table})
        assert not np.array_equal(moved, plain), name
        got = dff_traces_device(path, rois, WINDOW, percentile=Q, kind='num', chunk_frames=7, **{name: table})
        assert np.array_equal(got, moved), name
        got = dff_traces_device(path, rois, WINDOW, percentile=Q, kind='dff', chunk_frames=7, **{name: table})
        assert np.array_equal(_bits(got), _bits(ref.dff(moved, ref.baseline(moved, WINDOW // 2, Q)))), name


def test_neuropil_correction_recovers_a_planted_signal_exactly(tmp_path):
    """ROI pixels hold s_t + 3 n_t / 4 with n_t a multiple of 4, ring pixels hold n_t, weight 0.75 (a = 192): then
    N == 256 An A s_t exactly and 'f' == s_t bit for bit.  An ROI whose ring is empty (fenced in) gets N = S + o A."""
    from deep_calcium_amd import dff_traces_device, neuropil_rois
    rs = np.random.RandomState(8)
    T, H, W = 60, 24, 20
    n = 4 * rs.randint(10, 200, size=T)
    s = rs.randint(100, 4000, size=(2, T))
    centre = np.array([[12, 10]])
    fence = np.argwhere(np.ones((H, W)))
    d = np.maximum(np.abs(fence[:, 0] - 12), np.abs(fence[:, 1] - 10))
    fence = fence[(d >= 2) & (d <= 3)]                                        # a closed band around `centre`
    lone = np.argwhere(np.ones((3, 2))) + [2, 2]
    rois = [lone, centre, fence]
    inner, outer = 1, 3
    rings = neuropil_rois(rois, (H, W), inner, outer)
    assert len(rings[0]) > 0 and len(rings[1]) == 0 and len(rings[2]) > 0
    raw = np.broadcast_to(n[:, None, None], (T, H, W)).copy()                 # every pixel outside an ROI is neuropil
    raw[:, lone[:, 0], lone[:, 1]] = (s[0] + 3 * n // 4)[:, None]
    raw[:, fence[:, 0], fence[:, 1]] = (s[1] + 3 * n // 4)[:, None]
    raw[:, 12, 10] = rs.randint(0, 5000, size=T)
    raw = raw.astype(np.uint16)
    path = str(tmp_path / 'planted.npz')
    np.savez(path, series_raw=raw)
    args = dict(window=21, percentile=Q, neuropil=(inner, outer, 0.75), chunk_frames=16)
    N = dff_traces_device(path, rois, kind='num', **args)
    A, An = [len(c) for c in rois], [len(c) for c in rings]
    assert np.array_equal(N[0], 256 * An[0] * A[0] * s[0]) and np.array_equal(N[2], 256 * An[2] * A[2] * s[1])
    assert np.array_equal(N[1], raw[:, 12, 10].astype(np.int64))              # no ring: N = S
    f = dff_traces_device(path, rois, kind='f', **args)
    assert np.array_equal(_bits(f[0]), _bits(s[0].astype(np.float32))) and np.array_equal(_bits(f[2]), _bits(s[1].astype(np.float32)))
    assert np.array_equal(_bits(f[1]), _bits(raw[:, 12, 10].astype(np.float32)))
    N = dff_traces_device(path, rois, kind='num', offset=-7, **args)
    assert np.array_equal(N[1], raw[:, 12, 10].astype(np.int64) - 7)          # N = S + o A
    assert np.array_equal(N[0], 256 * An[0] * A[0] * s[0] - 7 * A[0] * An[0] * 64)
    want = ref.dff(N, ref.baseline(N, 10, Q))
    assert np.array_equal(_bits(dff_traces_device(path, rois, kind='dff', offset=-7, **args)), _bits(want))


def test_offset_lifts_a_negative_baseline(tmp_path):
    from deep_calcium_amd import dff_traces_device
    raw, rois = _recording(np.int16, seed=2)
    path = str(tmp_path / 'rec.npz')
    np.savez(path, series_raw=raw)
    without, _ = _oracle(raw, rois)
    assert (without['baseline_sum'] <= 0).all() and (_bits(without['dff']) == 0).all()
    lifted, _ = _oracle(raw, rois, offset=1600)
    assert (lifted['baseline_sum'] > 0).all() and (lifted['dff'] != 0).any()
    for offset, want in ((0, without), (1600, lifted)):
        for kind in ('baseline_sum', 'dff', 'f'):
            _same(dff_traces_device(path, rois, WINDOW, percentile=Q, kind=kind, offset=offset), want[kind], (offset, kind))
