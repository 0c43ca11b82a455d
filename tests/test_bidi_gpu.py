"""Bidirectional scan-phase correction on the device (include/dcunet.h dc_bidi_scores / dc_bidi_apply; BidiEstimator,
estimate_bidi_device, bidi= of MotionCorrector, make_template, estimate_shifts_device and the readers) against the integer oracle
of tests/_bidi_ref.py.  Every comparison is equality; every output buffer is pre-filled with garbage with a guard behind it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _bidi_ref as bref              # noqa: E402
import _gridcaps as caps              # noqa: E402
import _motion_ref as ref             # noqa: E402

DTYPES = [np.int16, np.uint16]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _rand(rs, shape, dtype):
    info = np.iinfo(dtype)
    return rs.randint(info.min, info.max + 1, size=shape).astype(dtype)


def _scores(L, frames, P, odd=0):
    """dc_bidi_scores into a table of garbage with a guard behind it; odd: the frames start that many elements into their
    allocation (off 16-byte alignment)."""
    T, H, W = frames.shape
    nd = 2 * P + 1
    src = torch.zeros((frames.size + odd + 8,), dtype=torch.int16, device='cuda')
    src[odd:odd + frames.size] = _dev(frames).reshape(-1)
    sc = torch.full((T * nd + 4,), -7, dtype=torch.int64, device='cuda')
    L.dc_bidi_scores(src.data_ptr() + 2 * odd, int(frames.dtype == np.uint16), T, H, W, P, sc.data_ptr(), _st())
    got = sc.cpu().numpy()
    assert (got[T * nd:] == -7).all()
    return got[:T * nd].reshape(T, nd)


def _apply(L, frames, p, fill=0, odd=0, odd_out=0):
    """dc_bidi_apply into a buffer of 0x5a5a with a guard on both sides; odd / odd_out: frames / out start that many elements into
    their allocation."""
    src = torch.zeros((frames.size + odd + 8,), dtype=torch.int16, device='cuda')
    src[odd:odd + frames.size] = _dev(frames).reshape(-1)
    buf = torch.full((frames.size + odd_out + 8,), 0x5a5a, dtype=torch.int16, device='cuda')
    T, H, W = frames.shape
    L.dc_bidi_apply(src.data_ptr() + 2 * odd, T, int(p), H, W, int(fill), buf.data_ptr() + 2 * odd_out, _st())
    got = buf.cpu().numpy()
    assert (got[:odd_out] == 0x5a5a).all() and (got[odd_out + frames.size:] == 0x5a5a).all()      # nothing around `out` is written
    return got[odd_out:odd_out + frames.size].reshape(frames.shape).view(frames.dtype)


# ---- dc_bidi_scores -----------------------------------------------------------------------------------------------------------------
# H: 3 and 4 (one odd row; 4 drops its last odd row), 5 (two rows of one wave), 9 (a whole wave), 11 (a second wave), 35 and 36 (a
# second row tile; 36 drops its last odd row).  W: one interior column, a ragged lane, a second column tile.
@pytest.mark.parametrize('P', [0, 1, 8, 16])
@pytest.mark.parametrize('dtype', DTYPES)
def test_scores_equal_the_oracle(dclib, P, dtype):
    rs = np.random.RandomState(100 + P)
    for H in (3, 4, 5, 9, 11, 35, 36):
        for W in (2 * P + 1, 2 * P + 8 * 2 + 3, 2 * P + 512 + 5):
            frames = _rand(rs, (3, H, W), dtype)
            want = bref.scores(frames, P)
            assert np.array_equal(_scores(dclib, frames, P), want), (H, W)
            assert np.array_equal(_scores(dclib, frames, P, odd=1), want), (H, W)      # one element off 16-byte alignment


@pytest.mark.parametrize('dtype', DTYPES)
def test_scores_of_the_extreme_frame_need_34_bits(dclib, dtype):
    info = np.iinfo(dtype)
    for P, H, W in ((0, 3, 1), (2, 9, 30), (16, 37, 600)):
        for odd_v, even_v in ((info.min, info.max), (info.max, info.min)):
            f = np.empty((2, H, W), dtype)
            f[:, 0::2] = even_v
            f[:, 1::2] = odd_v
            want = bref.scores(f, P)
            assert want[0, 0] == ((H - 1) // 2) * (W - 2 * P) * 131070 ** 2 and 131070 ** 2 >= 2 ** 33
            assert np.array_equal(_scores(dclib, f, P), want)


def test_scores_of_no_frame_write_nothing_and_bad_sizes_are_refused(dclib):
    from deep_calcium_amd._lib import DcunetError
    sc = torch.full((64,), -7, dtype=torch.int64, device='cuda')
    fr = torch.zeros((64,), dtype=torch.int16, device='cuda')
    assert dclib.dc_bidi_scores(fr.data_ptr(), 0, 0, 3, 5, 1, sc.data_ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert (sc.cpu().numpy() == -7).all()
    for H, W, P, code in ((2, 9, 1, -1), (3, 2, 1, -1), (3, 32, 16, -1), (3, 9, -1, -1), (9, 99, 17, -3), (2 ** 14, 2 ** 14 + 1, 2, -3)):
        with pytest.raises(DcunetError, match=r'\(%d\)' % code):
            dclib.dc_bidi_scores(fr.data_ptr(), 0, 1, H, W, P, sc.data_ptr(), _st())
    torch.cuda.synchronize()
    assert (sc.cpu().numpy() == -7).all()


@pytest.mark.parametrize('dtype', DTYPES)
def test_scores_past_the_frame_cap(dclib, dtype):
    rs = np.random.RandomState(7)
    base = caps.base_frames(rs, (3, 5), dtype)
    n = caps.TWO_TRIPS
    assert caps.first_stride_trip(n, caps.FRAME_CAP) is not None
    got = _scores(dclib, caps.expand(base, n), 1)
    assert np.array_equal(got, caps.expand(bref.scores(base, 1), n))


# ---- dc_bidi_apply ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tc,H,W', [(3, 5, 13), (2, 6, 24), (3, 4, 8), (2, 7, 40)])
@pytest.mark.parametrize('dtype', DTYPES)
def test_apply_equals_the_oracle(dclib, tc, H, W, dtype):
    rs = np.random.RandomState(H * W)
    frames = _rand(rs, (tc, H, W), dtype)
    for p in (0, 1, -1, W - 1, -(W - 1), W, -W, W + 5, -(W + 5), 3, -2):
        for fill in (0, -32768, 65535):
            want = bref.apply(frames, p, fill)
            if p == 0:
                assert np.array_equal(want, frames)
            for odd, odd_out in ((0, 0), (1, 0), (0, 1), (3, 5)):
                assert np.array_equal(_apply(dclib, frames, p, fill, odd, odd_out), want), (p, fill, odd, odd_out)


def test_apply_refuses_overlap_and_takes_any_int32(dclib):
    from deep_calcium_amd._lib import DcunetError
    buf = torch.zeros((4 * 6 * 10 + 16,), dtype=torch.int16, device='cuda')
    for delta in (0, 2, 2 * (2 * 6 * 10) - 2):
        with pytest.raises(DcunetError, match=r'\(-1\).*out overlaps frames'):
            dclib.dc_bidi_apply(buf.data_ptr(), 2, 1, 6, 10, 0, buf.data_ptr() + delta, _st())
    with pytest.raises(DcunetError, match=r'\(-1\).*fill'):
        dclib.dc_bidi_apply(buf.data_ptr(), 1, 1, 6, 10, 65536, buf.data_ptr() + 2 * 60, _st())
    rs = np.random.RandomState(1)
    frames = _rand(rs, (2, 5, 9), np.int16)
    for p in (2 ** 31 - 1, -2 ** 31):
        assert np.array_equal(_apply(dclib, frames, p, 7), bref.apply(frames, p, 7))


def test_apply_past_the_x_cap(dclib):
    """One frame of more than 8 * 4096 * 256 values: the groups of the last rows are reached on a second trip of the x grid."""
    H, W = caps.BIG_H, caps.BIG_W
    first, last = caps.apply_second_trip_rows(H, W, 1)
    assert first >= H - caps.BIG_BAND and last == H - 1
    rs = np.random.RandomState(5)
    frames = _rand(rs, (1, H, W), np.int16)
    got = _apply(dclib, frames, 3, -1)
    want = bref.apply(frames, 3, -1)
    assert H - 2 >= first and (want[0, H - 2, -3:] == -1).all() and np.array_equal(got[0, first:], want[0, first:])
    assert np.array_equal(got, want)


# ---- BidiEstimator, estimate_bidi_device ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_estimator_is_chunking_invariant(dtype):
    from deep_calcium_amd import BidiEstimator
    rs = np.random.RandomState(11)
    T, H, W, P = 19, 13, 37, 5
    frames = _rand(rs, (T, H, W), dtype)
    want = bref.scores(frames, P)
    one = BidiEstimator((H, W), dtype, max_offset=P).feed(frames)
    assert one.fed == T and np.array_equal(one.scores(), want) and one.scores().dtype == np.int64
    assert one.totals() == bref.totals(want) and one.offset() == bref.pick(bref.totals(want))
    parts = BidiEstimator((H, W), dtype, max_offset=P, chunk_frames=4)
    parts.feed(frames[:1]).feed(frames[1:8]).feed(frames[8:])
    assert np.array_equal(parts.scores(), want)
    res = BidiEstimator((H, W), dtype, max_offset=P, chunk_frames=5).feed(_dev(frames))
    assert np.array_equal(res.scores(), want)


def _write(path, frames):
    from deep_calcium_amd import hdf5_min
    w = hdf5_min.Writer()
    w.create_dataset('series/raw', data=frames)
    w.save(str(path))
    return str(path)


def test_estimate_bidi_device_recovers_the_planted_offsets(tmp_path):
    from deep_calcium_amd import estimate_bidi_device
    for i, (H, W, P, blobs, sigma, n, _) in enumerate(bref.CONFIGS + [bref.NOISY]):
        for b in (-(P - 1), -1, 0, 2, P - 1):
            frames = bref.planted(0, H, W, P, blobs, sigma, n, b)
            path = _write(tmp_path / ('planted_%d_%d.hdf5' % (i, b + P)), frames)
            offset, totals = estimate_bidi_device(path, max_offset=P)
            want = bref.totals(bref.scores(frames, P))
            assert totals == want and offset == bref.pick(want) == -b, (H, W, P, b)
    # frames=: the first frames only; None: all of them
    H, W, P, blobs, sigma, n, _ = bref.NOISY
    frames = bref.planted(1, H, W, P, blobs, sigma, n, 3)
    path = _write(tmp_path / 'first.hdf5', frames)
    assert estimate_bidi_device(path, max_offset=P, frames=2)[1] == bref.totals(bref.scores(frames[:2], P))
    assert estimate_bidi_device(path, max_offset=P, frames=None)[1] == bref.totals(bref.scores(frames, P))


# ---- MotionCorrector(bidi=), make_template(bidi=) ---------------------------------------------------------------------------------
def _moving(seed, T, H, W, S, b, dtype=np.int16):
    """T frames cut from one blob scene at random offsets within +-S, noise added, then the odd rows cut at the planted offset b."""
    rs = np.random.RandomState(seed)
    P = abs(b)
    img = np.rint(bref.scene(rs, H + 2 * S, W + 2 * S, 30, P)).astype(np.int64)
    offs = [(int(rs.randint(-S, S + 1)), int(rs.randint(-S, S + 1))) for _ in range(T)]
    out = np.empty((T, H, W), np.int64)
    for t, (a, c) in enumerate(offs):
        full = img[S + a:S + a + H] + rs.randint(-10, 11, size=(H, img.shape[1]))
        out[t] = full[:, P + S + c:P + S + c + W]
        out[t, 1::2] = full[1::2, P + S + c + b:P + S + c + b + W]
    return out.astype(dtype), np.array(offs)


MODES = [dict(), dict(blocks=(2, 2), max_dev=2), dict(subpixel=True), dict(max_shift=8, coarse=2)]


@pytest.mark.parametrize('mode', MODES, ids=['rigid', 'blocks', 'subpixel', 'coarse'])
def test_corrector_with_bidi_equals_a_corrector_fed_corrected_lines(mode):
    from deep_calcium_amd import MotionCorrector
    T, H, W, p, fill = 9, 40, 56, -3, -5
    frames, _ = _moving(3, T, H, W, 3, 3)
    lines = bref.apply(frames, p, fill)
    tmpl = ref.rounded_mean(lines)
    kw = dict(dict(max_shift=4, fill=fill, chunk_frames=4), **mode)
    a = MotionCorrector((H, W), T, np.int16, tmpl, bidi=p, **kw)
    b = MotionCorrector((H, W), T, np.int16, tmpl, **kw)
    assert a._bidi_scratch.shape == (4, H, W) and not hasattr(b, '_bidi_scratch') and b.bidi == 0
    for lo, hi in ((0, 1), (1, 7), (7, T)):
        ga, gb = a.feed(frames[lo:hi]), b.feed(lines[lo:hi])
        assert torch.equal(ga, gb)
        assert np.array_equal(a.last_scores(), b.last_scores())
        if 'blocks' in mode:
            assert np.array_equal(a.last_block_scores(), b.last_block_scores())
        if 'coarse' in mode:
            assert np.array_equal(a.last_coarse_scores(), b.last_coarse_scores())
    assert np.array_equal(a.shifts(), b.shifts()) and len(set(map(tuple, a.shifts().tolist()))) > 2
    if 'blocks' in mode:
        assert np.array_equal(a.block_shifts(), b.block_shifts())
    if 'subpixel' in mode:
        assert np.array_equal(a.fine_shifts(), b.fine_shifts())
    if 'coarse' in mode:
        assert np.array_equal(a.coarse_shifts(), b.coarse_shifts())
    # the valid rectangle: the plain one, narrowed by the line move
    (y0, y1), (x0, x1) = b.valid()
    (v0, v1), (u0, u1) = a.valid()
    assert (v0, v1) == (y0, y1) and u0 >= x0 and u1 <= x1 and (u0, u1) != (x0, x1)
    # a resident tensor is read in place and gives the same
    c = MotionCorrector((H, W), T, np.int16, tmpl, bidi=p, **kw)
    got = c.feed(_dev(frames))
    assert np.array_equal(c.shifts(), b.shifts()) and torch.equal(got[7:], gb)


def test_make_template_with_bidi():
    from deep_calcium_amd import make_template
    frames, _ = _moving(4, 12, 32, 48, 3, -2)
    for dtype in DTYPES:
        f = frames.astype(dtype)
        lines = bref.apply(f, 2, 0)
        for it in (0, 1):
            assert np.array_equal(make_template(f, max_shift=4, iterations=it, bidi=2), make_template(lines, max_shift=4, iterations=it))
        assert not np.array_equal(make_template(f, max_shift=4), make_template(lines, max_shift=4))
        assert np.array_equal(make_template(f, max_shift=4, bidi=0), make_template(f, max_shift=4))


# ---- the readers -------------------------------------------------------------------------------------------------------------------
def _rois(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return [np.stack([yy[m], xx[m]], 1) for m in ((yy - 9) ** 2 + (xx - 12) ** 2 <= 16, (yy - 20) ** 2 + (xx - 30) ** 2 <= 25,
                                                  (yy < 4) & (xx < 5))]


@pytest.mark.parametrize('with_shifts', [False, True], ids=['alone', 'with_shifts'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_readers_with_bidi_equal_readers_fed_corrected_lines(with_shifts, dtype):
    from deep_calcium_amd import RoiFootprints, RoiPairCorr, RoiTraceExtractor, SeriesSummarizer
    T, H, W, p = 11, 30, 44, 2
    frames, offs = _moving(5, T, H, W, 3, -2, dtype)
    lines = bref.apply(frames, p, 0)
    shifts = (-offs).astype(np.int32) if with_shifts else None
    rois = _rois(H, W)

    def both(make, result):
        a, b = make(bidi=p), make()
        a.feed(frames[:4]).feed(frames[4:])
        b.feed(lines)
        return result(a), result(b)
    kinds = ('mean', 'std', 'corr')
    ga, gb = both(lambda **k: SeriesSummarizer((H, W), T, dtype, kinds=kinds, chunk_frames=3, shifts=shifts, **k),
                  lambda s: [s.result(kind) for kind in kinds])
    for x, y in zip(ga, gb):
        assert np.array_equal(x, y)
    ga, gb = both(lambda **k: RoiTraceExtractor((H, W), T, dtype, rois, chunk_frames=3, shifts=shifts, **k), lambda s: s.result('sum'))
    assert np.array_equal(ga, gb) and ga.dtype == np.int64
    if not with_shifts:      # against numpy too: the sums of the oracle-corrected lines
        want = np.stack([lines.astype(np.int64)[:, r[:, 0], r[:, 1]].sum(axis=1) for r in rois])
        assert np.array_equal(ga, want)
        assert not np.array_equal(ga, np.stack([frames.astype(np.int64)[:, r[:, 0], r[:, 1]].sum(axis=1) for r in rois]))
    for cls in (RoiFootprints, RoiPairCorr):
        ga, gb = both(lambda **k: cls((H, W), T, dtype, rois, chunk_frames=3, shifts=shifts, **k), lambda s: s.result('moments'))
        assert len(ga) == len(gb) == len(rois)
        for x, y in zip(ga, gb):
            assert sorted(x) == sorted(y)
            for key in x:
                assert np.array_equal(x[key], y[key]), (cls.__name__, key)


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def test_end_to_end_on_a_dataset_file(tmp_path):
    from deep_calcium_amd import estimate_bidi_device, estimate_shifts_device, extract_traces_device, summarize_series_device
    # planted shifts within +-4 searched within +-8: the line move leaves |p| columns of fill at one edge of the odd lines, which the
    # search reads as a mismatch at every shift that reaches them -- max_shift >= the largest shift + |p| keeps the true one clear
    T, H, W, S = 40, 32, 64, 8
    frames, offs = _moving(9, T, H, W, 4, -3)
    assert np.abs(offs).max() == 4
    path = _write(tmp_path / 'raw.hdf5', frames)
    offset, totals = estimate_bidi_device(path, max_offset=8)
    assert offset == 3 == bref.pick(bref.totals(bref.scores(frames, 8))) and totals == bref.totals(bref.scores(frames, 8))
    shifts, tmpl = estimate_shifts_device(path, max_shift=S, bidi=3)
    lines = bref.apply(frames, 3, 0)
    want_t = ref.make_template(lines, S, 1)
    assert np.array_equal(tmpl, want_t) and np.array_equal(shifts, ref.pick(ref.scores(lines, want_t, S)))
    assert np.array_equal(shifts, -offs)                                   # every planted shift
    # bidi=0: the numpy oracle on the uncorrected frames
    plain, tmpl0 = estimate_shifts_device(path, max_shift=S, bidi=0)
    raw_t = ref.make_template(frames, S, 1)
    assert np.array_equal(tmpl0, raw_t) and np.array_equal(plain, ref.pick(ref.scores(frames, raw_t, S)))
    # the one-call readers take both corrections
    cpath = _write(tmp_path / 'corrected.hdf5', ref.apply(lines, shifts, 0))
    for kind in ('mean', 'corr'):
        assert np.array_equal(summarize_series_device(path, kind=kind, shifts=shifts, bidi=3), summarize_series_device(cpath, kind=kind))
    rois = _rois(H, W)
    assert np.array_equal(extract_traces_device(path, rois, kind='sum', shifts=shifts, bidi=3), extract_traces_device(cpath, rois, kind='sum'))
