"""Frame quality on the device (include/dcunet.h dc_frame_moments, dc_frame_quality, dc_frame_gather; FrameQuality, FrameFilter;
keep= of the one-call functions) against the naive oracle of tests/_frames_ref.py.  Every comparison is equality; every output
buffer is pre-filled with a pattern and has a guard on both sides."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _bidi_ref as bref              # noqa: E402
import _frames_ref as ref             # noqa: E402
import _motion_ref as mref            # noqa: E402
import _pair_ref as pref              # noqa: E402
import _tbin_ref as tref              # noqa: E402

DTYPES = [np.int16, np.uint16]
PATTERN, GARBAGE = 0x5a5a, 0x7b7b7b7b7b7b7b7b
FRAME_CAP = 1024                      # frames one trip of the y grid of dc_frame_moments / dc_frame_gather covers (kMaxFrames)
QUALITY_CAP = 1024 * 256              # frames one trip of dc_frame_quality covers (kMaxFrames workgroups of 256 threads)
SLAB_ROWS, SLAB_CAP = 32, 1024        # rows of a slab, slabs one trip of the x grid of dc_frame_moments covers
GATHER_X_CAP = 1024 * 256 * 8         # pixels of a frame one trip of the x grid of dc_frame_gather covers


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _rand(rs, shape, dtype):
    info = np.iinfo(dtype)
    return rs.randint(info.min, info.max + 1, size=shape).astype(dtype)


def _offset(a, odd):
    """The values of `a` starting `odd` elements into a 16-byte aligned allocation -> (the allocation, the pointer)."""
    buf = torch.zeros((a.size + odd + 8,), dtype=torch.int16, device='cuda')
    buf[odd:odd + a.size] = _dev(a).reshape(-1)
    assert buf.data_ptr() % 16 == 0
    return buf, buf.data_ptr() + 2 * odd


def _moments(L, frames, tmpl=None, rect=None, odd=0, odd_t=0):
    """One dc_frame_moments call -> int64 (tc, 3).  moments: a buffer of garbage (the call must zero its rows itself) with a guard
    on both sides.  odd / odd_t: frames / tmpl start that many elements into their 16-byte aligned allocation."""
    tc, H, W = frames.shape
    (y0, y1), (x0, x1) = ref.rect_of((H, W), rect)
    src, fp = _offset(frames, odd)
    tbuf, tp = (None, None) if tmpl is None else _offset(tmpl, odd_t)
    buf = torch.full((2 + 3 * tc + 2,), GARBAGE, dtype=torch.int64, device='cuda')
    L.dc_frame_moments(fp, int(frames.dtype == np.uint16), tc, tp, H, W, y0, y1, x0, x1, buf.data_ptr() + 16, _st())
    got = buf.cpu().numpy()
    assert (got[:2] == GARBAGE).all() and (got[2 + 3 * tc:] == GARBAGE).all()            # nothing around `moments` is written
    return got[2:2 + 3 * tc].reshape(tc, 3)


def _quality(L, mom, n, ta, tb, with_corr=True):
    """One dc_frame_quality call on the int64 (tc, 3) moments -> (mean, corr or None) float32 (tc,), guards checked."""
    tc = mom.shape[0]
    m = torch.from_numpy(np.ascontiguousarray(mom)).cuda()
    mean = torch.full((4 + tc + 4,), float('nan'), dtype=torch.float32, device='cuda')
    corr = torch.full((4 + tc + 4,), float('nan'), dtype=torch.float32, device='cuda')
    L.dc_frame_quality(m.data_ptr(), tc, n, ta, tb, mean.data_ptr() + 16, corr.data_ptr() + 16 if with_corr else None, _st())
    mean, corr = mean.cpu().numpy(), corr.cpu().numpy()
    for v in (mean, corr):
        assert np.isnan(v[:4]).all() and np.isnan(v[4 + tc:]).all()
    if not with_corr:
        assert np.isnan(corr).all()
        return mean[4:4 + tc], None
    return mean[4:4 + tc], corr[4:4 + tc]


def _same_bits(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _check_scores(L, frames, tmpl, rect, **odd):
    """moments, mean and corr of one call chain against the oracle, bit for bit."""
    want_m, want_mean, want_corr = ref.scores(frames, tmpl, rect)
    got_m = _moments(L, frames, tmpl, rect, **odd)
    where = (frames.dtype, frames.shape, rect, odd)
    assert np.array_equal(got_m, want_m), where
    n = ref.n_pixels(frames.shape[1:], rect)
    if tmpl is None:
        mean, corr = _quality(L, got_m, n, 0, 0, with_corr=False)
        assert _same_bits(mean, want_mean) and (got_m[:, 2] == 0).all(), where
        return got_m, mean, None
    ta, tb, tc_ = _moments(L, tmpl[None], None, rect)[0]
    assert (int(ta), int(tb), int(tc_)) == ref.moments(tmpl[None], None, rect)[0], where
    mean, corr = _quality(L, got_m, n, int(ta), int(tb))
    assert _same_bits(mean, want_mean) and _same_bits(corr, want_corr), (where, corr, want_corr)
    return got_m, mean, corr


def _edgy(rs, shape, dtype):
    """Random frames with both extremes of the type planted in every frame."""
    info = np.iinfo(dtype)
    f = _rand(rs, shape, dtype)
    flat = f.reshape(shape[0], -1)
    flat[:, 0] = info.max
    if flat.shape[1] > 1:
        flat[:, -1] = info.min
    return f


# ---- dc_frame_moments / dc_frame_quality ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_moments_and_scores_equal_the_oracle(dclib, dtype):
    rs = np.random.RandomState(20 + int(dtype == np.uint16))
    # 5 x 7: smaller than a wave, no 16-byte word in a row unless it happens to be aligned
    frames, tmpl = _edgy(rs, (3, 5, 7), dtype), _rand(rs, (5, 7), dtype)
    for odd, odd_t in ((0, 0), (1, 0), (0, 3), (5, 5)):
        _check_scores(dclib, frames, tmpl, None, odd=odd, odd_t=odd_t)
        _check_scores(dclib, frames, None, None, odd=odd)
    _check_scores(dclib, frames, tmpl, ((1, 4), (2, 6)))
    # 33 x 65: more than one slab of rows, rows of 8 words and a tail; rectangles that start at an odd x0, of width 1 and 2, one pixel
    frames, tmpl = _edgy(rs, (3, 33, 65), dtype), _rand(rs, (33, 65), dtype)
    rects = (None, ((0, 33), (1, 65)), ((2, 33), (3, 64)), ((0, 33), (7, 8)), ((1, 32), (63, 65)), ((5, 6), (0, 65)), ((32, 33), (64, 65)),
             ((0, 1), (0, 1)), ((0, 33), (9, 33)))
    for rect in rects:
        for odd, odd_t in ((0, 0), (1, 1), (0, 1), (3, 6), (7, 0)):                     # the template's rows share the frame rows' alignment, or not
            _check_scores(dclib, frames, tmpl, rect, odd=odd, odd_t=odd_t)
        _check_scores(dclib, frames, None, rect, odd=2)
    # a row of exactly one lane's word per lane and more: 1 x 520, 2 x 1031
    for shape in ((2, 1, 520), (2, 2, 1031)):
        frames, tmpl = _edgy(rs, shape, dtype), _rand(rs, shape[1:], dtype)
        _check_scores(dclib, frames, tmpl, None, odd=1, odd_t=1)
        _check_scores(dclib, frames, tmpl, ((0, shape[1]), (5, shape[2] - 3)))


def test_moments_of_a_frame_of_nothing_but_65535(dclib):
    """192 x 192 uint16, every pixel 65535: 36 864 pixels, so an int32 sum of x overflows, and every square needs 33 bits."""
    frames = np.full((2, 192, 192), 65535, np.uint16)
    frames[1, 100, 7] = 0
    tmpl = np.full((192, 192), 65535, np.uint16)
    got = _moments(dclib, frames, tmpl)
    n = 192 * 192
    assert got[0].tolist() == [n * 65535, n * 65535 ** 2, n * 65535 ** 2] and n * 65535 > 2 ** 31 and 65535 ** 2 > 2 ** 31
    assert got[1].tolist() == [(n - 1) * 65535, (n - 1) * 65535 ** 2, (n - 1) * 65535 ** 2]
    mean, corr = _quality(dclib, got, n, n * 65535, n * 65535 ** 2)
    assert mean[0] == np.float32(65535) and corr.tolist() == [0.0, 0.0]                  # a constant template: exactly 0
    rs = np.random.RandomState(3)
    _check_scores(dclib, frames, _rand(rs, (192, 192), np.uint16), None)
    # and the other end of the other type
    low = np.full((1, 192, 192), -32768, np.int16)
    got = _moments(dclib, low, low[0])
    assert got[0].tolist() == [-n * 32768, n * 32768 ** 2, n * 32768 ** 2]


@pytest.mark.parametrize('dtype', DTYPES)
def test_more_frames_than_any_grid_holds(dclib, dtype):
    """2 x 3 frames, tc past the frame cap of dc_frame_moments (1024 workgroup rows) and past the cap of dc_frame_quality (1024
    workgroups of 256 frames): the frames of the second trips are distinct from those of the first."""
    rs = np.random.RandomState(30 + int(dtype == np.uint16))
    base = _edgy(rs, (61, 2, 3), dtype)                                              # 61 is coprime to both caps
    tmpl = _rand(rs, (2, 3), dtype)
    tc = QUALITY_CAP + 7
    assert tc > FRAME_CAP and tc % 61 != 0
    frames = np.ascontiguousarray(base[np.arange(tc) % 61])
    want_m, want_mean, want_corr = ref.scores(base, tmpl, None)
    pick = np.arange(tc) % 61
    got_m = _moments(dclib, frames, tmpl)
    assert np.array_equal(got_m[FRAME_CAP], want_m[FRAME_CAP % 61]) and np.array_equal(got_m, want_m[pick])
    (ta, tb, _), = ref.moments(tmpl[None])
    mean, corr = _quality(dclib, got_m, 6, ta, tb)
    assert _same_bits(mean[QUALITY_CAP:], want_mean[pick][QUALITY_CAP:]) and _same_bits(mean, want_mean[pick])
    assert _same_bits(corr, want_corr[pick])


def test_more_rows_than_the_slab_grid_holds(dclib):
    """A rectangle of more than 1024 slabs of 32 rows, 2 columns wide: the last slabs are reached on a second trip of the x grid."""
    H = SLAB_ROWS * SLAB_CAP + 37
    rs = np.random.RandomState(31)
    frames, tmpl = _edgy(rs, (2, H, 2), np.int16), _rand(rs, (H, 2), np.int16)
    frames[:, SLAB_ROWS * SLAB_CAP:] = 32767                                         # the second trip is not a small correction
    _check_scores(dclib, frames, tmpl, None)
    _check_scores(dclib, frames, tmpl, ((3, H), (1, 2)), odd=1)


@pytest.mark.parametrize('dtype', DTYPES)
def test_the_exact_cases_of_the_correlation(dclib, dtype):
    rs = np.random.RandomState(40)
    H, W = 9, 21
    tmpl = rs.randint(0, 2000, size=(H, W)).astype(dtype)
    k = 2500
    frames = np.stack([tmpl, (k - tmpl.astype(np.int64)).astype(dtype), np.full((H, W), 77, dtype), (tmpl.astype(np.int64) + 5).astype(dtype)])
    for rect in (None, ((1, 8), (3, 20))):
        got_m, mean, corr = _check_scores(dclib, frames, tmpl, rect, odd=1)
        assert corr.view(np.uint32).tolist() == [np.float32(v).view(np.uint32) for v in (1.0, -1.0, 0.0, 1.0)], corr
        assert mean[2] == np.float32(77)
    # one pixel: nothing varies; a constant template: 0 for every frame
    _, _, corr = _check_scores(dclib, frames, tmpl, ((4, 5), (6, 7)))
    assert (corr.view(np.uint32) == 0).all()
    _, _, corr = _check_scores(dclib, frames, np.full((H, W), 9, dtype), None)
    assert (corr.view(np.uint32) == 0).all()
    # tmpl = NULL leaves c == 0
    assert (_moments(dclib, frames)[:, 2] == 0).all()


def test_bad_arguments_are_refused_by_the_entry_points_and_nothing_is_launched(dclib):
    from deep_calcium_amd._lib import DcunetError
    L = dclib
    fr = torch.full((256,), 3, dtype=torch.int16, device='cuda')
    mom = torch.full((64,), GARBAGE, dtype=torch.int64, device='cuda')
    out = torch.full((256,), PATTERN, dtype=torch.int16, device='cuda')
    fl = torch.full((64,), 7.0, dtype=torch.float32, device='cuda')
    idx = torch.zeros((16,), dtype=torch.int32, device='cuda')
    f, m, o, x, i = fr.data_ptr(), mom.data_ptr(), out.data_ptr(), fl.data_ptr(), idx.data_ptr()

    def refused(code, text, fn, *args):
        with pytest.raises(DcunetError, match=r'\(%d\).*%s' % (code, text)):
            fn(*(args + (_st(),)))
    # dc_frame_moments
    refused(-3, 'limited to 2.28', L.dc_frame_moments, f, 0, 1, None, 2 ** 15, 2 ** 14, 0, 2 ** 15, 0, 2 ** 14, m)           # n = 2^29
    refused(-3, 'limited to 2.28', L.dc_frame_moments, f, 1, 1, f, 2 ** 15, 2 ** 15, 0, 2 ** 14, 1, 2 + 2 ** 14, m)           # n = 2^28 + 2^14
    refused(-3, 'limited to 2.30', L.dc_frame_moments, f, 0, 1, None, 2 ** 16, 2 ** 15, 0, 1, 0, 1, m)
    refused(-1, 'null pointer', L.dc_frame_moments, None, 0, 2, None, 3, 5, 0, 3, 0, 5, m)
    refused(-1, 'null pointer', L.dc_frame_moments, f, 0, 2, None, 3, 5, 0, 3, 0, 5, None)
    refused(-1, 'misaligned', L.dc_frame_moments, f + 1, 0, 2, None, 3, 5, 0, 3, 0, 5, m)
    refused(-1, 'misaligned', L.dc_frame_moments, f, 0, 2, f + 31, 3, 5, 0, 3, 0, 5, m)
    refused(-1, 'misaligned', L.dc_frame_moments, f, 0, 2, None, 3, 5, 0, 3, 0, 5, m + 4)
    refused(-1, 'negative or zero size', L.dc_frame_moments, f, 0, -1, None, 3, 5, 0, 3, 0, 5, m)
    refused(-1, 'negative or zero size', L.dc_frame_moments, f, 0, 2, None, 0, 5, 0, 0, 0, 5, m)
    for rect in ((0, 4, 0, 5), (0, 3, 0, 6), (-1, 3, 0, 5), (0, 3, -1, 5), (2, 2, 0, 5), (0, 3, 4, 3)):
        refused(-1, 'empty or leaves', L.dc_frame_moments, f, 0, 2, None, 3, 5, rect[0], rect[1], rect[2], rect[3], m)
    assert L.dc_frame_moments(f, 0, 0, None, 3, 5, 0, 3, 0, 5, m, _st()) == 0                                        # tc == 0: nothing
    # dc_frame_quality
    refused(-3, 'limited to 2.28', L.dc_frame_quality, m, 2, 2 ** 28 + 1, 0, 0, x, x + 32)
    refused(-1, 'n = 0', L.dc_frame_quality, m, 2, 0, 0, 0, x, None)
    refused(-1, 'null pointer', L.dc_frame_quality, None, 2, 15, 0, 0, x, None)
    refused(-1, 'null pointer', L.dc_frame_quality, m, 2, 15, 0, 0, None, x)
    refused(-1, 'misaligned', L.dc_frame_quality, m + 4, 2, 15, 0, 0, x, None)
    refused(-1, 'misaligned', L.dc_frame_quality, m, 2, 15, 0, 0, x + 2, None)
    refused(-1, 'misaligned', L.dc_frame_quality, m, 2, 15, 0, 0, x, x + 34)
    refused(-1, 'negative count', L.dc_frame_quality, m, -2, 15, 0, 0, x, None)
    assert L.dc_frame_quality(m, 0, 15, 0, 0, x, x + 32, _st()) == 0
    # dc_frame_gather
    refused(-1, 'null pointer', L.dc_frame_gather, None, 4, i, 2, 3, 5, o)
    refused(-1, 'null pointer', L.dc_frame_gather, f, 4, None, 2, 3, 5, o)
    refused(-1, 'null pointer', L.dc_frame_gather, f, 4, i, 2, 3, 5, None)
    refused(-1, 'misaligned', L.dc_frame_gather, f + 1, 4, i, 2, 3, 5, o)
    refused(-1, 'misaligned', L.dc_frame_gather, f, 4, i + 2, 2, 3, 5, o)
    refused(-1, 'misaligned', L.dc_frame_gather, f, 4, i, 2, 3, 5, o + 1)
    refused(-1, 'negative or zero size', L.dc_frame_gather, f, 4, i, -1, 3, 5, o)
    refused(-1, 'negative or zero size', L.dc_frame_gather, f, -4, i, 1, 3, 5, o)
    refused(-1, 'negative or zero size', L.dc_frame_gather, f, 4, i, 1, 3, 0, o)
    refused(-3, 'limited to 2.30', L.dc_frame_gather, f, 4, i, 1, 2 ** 16, 2 ** 15, o)
    refused(-1, 'out overlaps frames', L.dc_frame_gather, f, 4, i, 2, 3, 5, f + 2 * 59)
    assert L.dc_frame_gather(f, 4, i, 0, 3, 5, o, _st()) == 0 and L.dc_frame_gather(None, 4, None, 0, 3, 5, None, _st()) == 0        # k == 0: nothing
    torch.cuda.synchronize()
    assert (mom.cpu().numpy() == GARBAGE).all() and (out.cpu().numpy() == PATTERN).all() and (fl.cpu().numpy() == 7.0).all()
    assert (fr.cpu().numpy() == 3).all()


# ---- dc_frame_gather --------------------------------------------------------------------------------------------------------------
def _gather(L, frames, idx, odd=0, odd_out=0):
    tc, H, W = frames.shape
    hw, k = H * W, len(idx)
    src, fp = _offset(frames, odd)
    lead = 8 + odd_out
    buf = torch.full((lead + k * hw + 8,), PATTERN, dtype=torch.int16, device='cuda')
    ix = torch.from_numpy(np.asarray(idx, np.int32).reshape(-1)).cuda()
    L.dc_frame_gather(fp, tc, ix.data_ptr() if k else None, k, H, W, buf.data_ptr() + 2 * lead, _st())
    got = buf.cpu().numpy()
    assert (got[:lead] == PATTERN).all() and (got[lead + k * hw:] == PATTERN).all()      # nothing around `out` is written
    return got[lead:lead + k * hw].reshape(k, H, W).view(frames.dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_gather_equals_the_oracle(dclib, dtype):
    rs = np.random.RandomState(50)
    for H, W in ((1, 1), (2, 3), (5, 7), (4, 8), (3, 520), (33, 65)):
        frames = _rand(rs, (9, H, W), dtype)
        frames[frames == 0] = 1                                                          # an all-zero frame is then a refused index, not data
        for idx in ([], list(range(9)), list(range(0, 9, 2)), [8, 8, 0, 3], [2, 9, -1, 4, 2 ** 31 - 1, -2 ** 31, 0]):
            want = ref.gather(frames, idx)
            for odd, odd_out in ((0, 0), (1, 0), (0, 1), (3, 5)):
                got = _gather(dclib, frames, idx, odd, odd_out)
                assert got.shape == want.shape and np.array_equal(got, want), (H, W, idx, odd, odd_out)
        assert (ref.gather(frames, [9, -1]) == 0).all() and (_gather(dclib, frames, [9, -1]) == 0).all()        # out of range: zero frames


def test_gather_past_both_grid_caps(dclib):
    rs = np.random.RandomState(51)
    frames = _rand(rs, (7, 2, 3), np.int16)
    idx = rs.randint(-1, 8, size=2 * FRAME_CAP + 5)                                      # more output frames than the y grid holds
    got = _gather(dclib, frames, idx)
    assert np.array_equal(got[FRAME_CAP:], ref.gather(frames, idx)[FRAME_CAP:]) and np.array_equal(got, ref.gather(frames, idx))
    W = GATHER_X_CAP + 8 * 300 + 5                                                       # more pixels than one trip of the x grid moves
    frames = _rand(rs, (2, 1, W), np.int16)
    for odd in (0, 1):
        got = _gather(dclib, frames, [1, 0], odd=odd)
        assert np.array_equal(got[:, :, GATHER_X_CAP:], frames[::-1][:, :, GATHER_X_CAP:]) and np.array_equal(got, frames[::-1])


# ---- FrameQuality / FrameFilter ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_quality_and_filter_are_chunking_invariant(dtype):
    from deep_calcium_amd import FrameFilter, FrameQuality
    rs = np.random.RandomState(60)
    T, H, W = 23, 5, 19
    frames, tmpl = _edgy(rs, (T, H, W), dtype), _rand(rs, (H, W), dtype)
    rect = ((1, 5), (3, 18))
    want_m, want_mean, want_corr = ref.scores(frames, tmpl, rect)
    keep = rs.rand(T) < 0.6
    keep[[0, 1, 2, 11]] = False, False, False, True                                      # a feed of 3 that keeps nothing
    kept = frames[keep]
    for step in (1, 3, 7, T):
        for resident in (False, True):
            fq = FrameQuality((H, W), T, dtype, template=_dev(tmpl) if resident else tmpl, rect=rect, chunk_frames=4)
            ff = FrameFilter((H, W), T, dtype, keep, chunk_frames=4)
            outs = []
            for a in range(0, T, step):
                part = frames[a:a + step]
                fq.feed(_dev(part) if resident else part)
                out = ff.feed(_dev(part) if resident else part)
                assert out.dtype == torch.int16 and out.is_cuda and out.is_contiguous() and tuple(out.shape[1:]) == (H, W)
                assert out.shape[0] == int(keep[a:a + step].sum())
                outs.append(out)
                assert fq.result('moments').shape == (fq.fed, 3)                         # the frames fed so far
            where = (step, resident)
            assert fq.result('moments').dtype == np.int64 and np.array_equal(fq.result('moments'), want_m), where
            assert _same_bits(fq.result('mean'), want_mean) and _same_bits(fq.result('corr'), want_corr), where
            assert np.array_equal(torch.cat(outs).cpu().numpy().view(dtype), kept), where
            assert (ff.n_out, ff.fed, ff.emitted) == (int(keep.sum()), T, int(keep.sum()))
    with pytest.raises(ValueError, match='after 23 fed'):
        ff.feed(frames[:1])
    with pytest.raises(ValueError, match='after 23 fed'):
        fq.feed(frames[:1])
    # no template: mean and moments with c == 0, and no corr
    fq = FrameQuality((H, W), T, dtype).feed(frames)
    want_m, want_mean, _ = ref.scores(frames, None, None)
    assert np.array_equal(fq.result('moments'), want_m) and _same_bits(fq.result('mean'), want_mean)
    with pytest.raises(ValueError, match='needs a template'):
        fq.result('corr')
    with pytest.raises(ValueError, match='kind'):
        fq.result('std')


def test_quality_and_filter_apply_the_corrections_first():
    from deep_calcium_amd import FrameFilter, FrameQuality
    rs = np.random.RandomState(61)
    T, H, W, p = 17, 12, 21, 2
    keep = rs.rand(T) < 0.5
    keep[3] = True
    for dtype in DTYPES:
        frames, tmpl = _rand(rs, (T, H, W), dtype), _rand(rs, (H, W), dtype)
        shifts = rs.randint(-3, 4, size=(T, 2)).astype(np.int32)
        lines = bref.apply(frames, p, 0)
        for kw, moved in ((dict(shifts=shifts, bidi=p), mref.apply(lines, shifts, 0)), (dict(bidi=p), lines),
                          (dict(shifts=shifts), mref.apply(frames, shifts, 0))):
            assert not np.array_equal(moved[keep], frames[keep])
            rect = ((3, 9), (5, 16))
            want_m, want_mean, want_corr = ref.scores(moved, tmpl, rect)
            for resident in (False, True):
                ff = FrameFilter((H, W), T, dtype, keep, chunk_frames=4, **kw)
                fq = FrameQuality((H, W), T, dtype, template=tmpl, rect=rect, chunk_frames=4, **kw)
                outs = []
                for a in range(0, T, 5):
                    part = _dev(frames[a:a + 5]) if resident else frames[a:a + 5]
                    outs.append(ff.feed(part))
                    fq.feed(part)
                where = (sorted(kw), resident)
                assert np.array_equal(torch.cat(outs).cpu().numpy().view(dtype), moved[keep]), where          # the rows of the table are the recording's
                assert np.array_equal(fq.result('moments'), want_m) and _same_bits(fq.result('corr'), want_corr), where
                assert _same_bits(fq.result('mean'), want_mean), where


# ---- the one-call functions, end to end --------------------------------------------------------------------------------------------
def _same_lists(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)


@pytest.fixture(scope='module')
def flashed(tmp_path_factory):
    """_pair_ref.gpu_scene() with three frames raised by 2000 grey levels -> dict(frames, rois, left, right, idx, path of the
    recording, path of a recording from which the flagged frames were removed on the host, keep as the device scores give it)."""
    from deep_calcium_amd import flag_frames, frame_quality_device
    clean, rois, left, right = pref.gpu_scene()
    frames, idx = ref.plant(clean, 7)
    root = tmp_path_factory.mktemp('flashed')
    path = str(root / 'flashed.npz')
    np.savez(path, series_raw=frames)
    tmpl = ref.template_of(frames)
    mean, corr = frame_quality_device(path, template=tmpl, chunk_frames=37)
    _, want_mean, want_corr = ref.scores(frames, tmpl, None, mom=ref.moments_np)
    assert _same_bits(mean, want_mean) and _same_bits(corr, want_corr)
    keep = flag_frames(mean, corr)
    assert np.flatnonzero(~keep).tolist() == idx.tolist()                                # the planted frames, and only they
    only_mean, none = frame_quality_device(path)
    assert none is None and _same_bits(only_mean, want_mean)
    removed = str(root / 'removed.npz')
    np.savez(removed, series_raw=frames[keep])
    return dict(frames=frames, rois=rois, left=left, right=right, idx=idx, path=path, removed=removed, keep=keep)


def test_keep_equals_a_recording_without_the_frames(flashed):
    from deep_calcium_amd import (merge_rois_device, roi_footprints_device, roi_pair_corr_device, split_rois_device,
                                  summarize_series_device)
    path, removed, keep, rois = flashed['path'], flashed['removed'], flashed['keep'], flashed['rois']
    # the flashes blind the split rule; leaving them out gives the two planted cells back
    new, origin, gaps = split_rois_device(path, rois)
    assert origin == [0, 1, 2, 3, 4] and gaps[1] < 0.05
    new, origin, gaps = split_rois_device(path, rois, keep=keep, chunk_frames=50)
    want = split_rois_device(removed, rois)
    assert origin == want[1] == [0, 1, 1, 2, 3, 4] and np.array_equal(gaps, want[2], equal_nan=True) and gaps[1] >= 0.2
    _same_lists(new, want[0])
    assert np.array_equal(new[1], flashed['left']) and np.array_equal(new[2], flashed['right'])
    got, want = roi_pair_corr_device(path, rois, keep=keep, chunk_frames=50), roi_pair_corr_device(removed, rois)
    _same_lists(got[0], want[0])
    _same_lists(got[1], want[1])
    got, want = roi_footprints_device(path, rois, keep=keep, chunk_frames=50), roi_footprints_device(removed, rois)
    for g, w in zip(got, want):
        _same_lists(g, w)
    for kind in ('mean', 'max', 'std', 'corr'):
        assert np.array_equal(summarize_series_device(path, kind=kind, keep=keep, chunk_frames=50), summarize_series_device(removed, kind=kind)), kind
    assert summarize_series_device(path, kind='max', standardize=False).max() > 2000 > summarize_series_device(path, kind='max', standardize=False, keep=keep).max()
    halves = [flashed['left'], flashed['right'], rois[3]]
    got, want = merge_rois_device(path, halves, keep=keep, chunk_frames=50), merge_rois_device(removed, halves)
    assert got[1] == want[1] and np.array_equal(got[2], want[2]) and len(got[2]) >= 1 and _same_bits(got[3], want[3])
    _same_lists(got[0], want[0])
    assert not _same_bits(got[3], merge_rois_device(path, halves)[3])


def test_a_keep_of_all_frames_is_none(flashed):
    from deep_calcium_amd import (merge_rois_device, roi_footprints_device, roi_pair_corr_device, split_rois_device,
                                  summarize_series_device)
    path, rois = flashed['path'], flashed['rois']
    every = np.ones(flashed['frames'].shape[0], bool)
    rs = np.random.RandomState(2)
    shifts = rs.randint(-2, 3, size=(len(every), 2)).astype(np.int32)
    for kw in ({}, dict(shifts=shifts, bidi=1), dict(detrend_frames=64), dict(bin_frames=3)):
        for kind in ('mean', 'std', 'corr'):
            assert np.array_equal(summarize_series_device(path, kind=kind, keep=every, **kw), summarize_series_device(path, kind=kind, **kw)), (kind, kw)
        _same_lists(roi_pair_corr_device(path, rois, keep=every, **kw)[0], roi_pair_corr_device(path, rois, **kw)[0])
        _same_lists(roi_footprints_device(path, rois, keep=every, **kw)[0], roi_footprints_device(path, rois, **kw)[0])
    got, want = split_rois_device(path, rois, keep=every), split_rois_device(path, rois)
    _same_lists(got[0], want[0])
    assert got[1] == want[1] and np.array_equal(got[2], want[2], equal_nan=True)
    halves = [flashed['left'], flashed['right']]
    for kw in ({}, dict(detrend_frames=64)):
        assert _same_bits(merge_rois_device(path, halves, keep=every, **kw)[3], merge_rois_device(path, halves, **kw)[3])


def test_keep_then_bin_then_detrend_equals_the_host_composition(flashed):
    """bidi, then shifts, then keep, then bin, then detrend: the readers see what the oracles give, composed on the host."""
    from deep_calcium_amd import RoiFootprints, RoiPairCorr, SeriesSummarizer, roi_footprints_device, roi_pair_corr_device, summarize_series_device
    frames, path, rois = flashed['frames'], flashed['path'], flashed['rois']
    T, H, W = frames.shape
    rs = np.random.RandomState(4)
    keep = flashed['keep'].copy()
    keep[rs.choice(T, 20, replace=False)] = False                                        # 233 or so frames stay: no multiple of b
    shifts = rs.randint(-2, 3, size=(T, 2)).astype(np.int32)
    b, L = 3, 16
    for kw, moved in ((dict(), frames), (dict(shifts=shifts, bidi=1), mref.apply(bref.apply(frames, 1, 0), shifts, 0))):
        binned = tref.bin_time(moved[keep], b)
        n = binned.shape[0]
        assert n == int(keep.sum()) // b and n > 2 * L
        for kind in ('std', 'corr', 'mean'):
            want = SeriesSummarizer((H, W), n, np.int16, kinds=(kind,), detrend_frames=L).feed(binned).result(kind, standardize=True)
            assert np.array_equal(summarize_series_device(path, kind=kind, keep=keep, bin_frames=b, detrend_frames=L, chunk_frames=41, **kw), want), kind
        pc = RoiPairCorr((H, W), n, np.int16, rois, detrend_frames=L).feed(binned)
        _same_lists(roi_pair_corr_device(path, rois, keep=keep, bin_frames=b, detrend_frames=L, chunk_frames=41, **kw)[0], pc.result('corr'))
        fp = RoiFootprints((H, W), n, np.int16, rois, detrend_frames=L).feed(binned)
        _same_lists(roi_footprints_device(path, rois, keep=keep, bin_frames=b, detrend_frames=L, chunk_frames=41, **kw)[0], fp.result('corr'))
        # keep and detrend without binning: L counts kept frames
        pc = RoiPairCorr((H, W), int(keep.sum()), np.int16, rois, detrend_frames=L).feed(np.ascontiguousarray(moved[keep]))
        _same_lists(roi_pair_corr_device(path, rois, keep=keep, detrend_frames=L, **kw)[0], pc.result('corr'))


def test_hold_index_patches_resident_sums(flashed):
    """sums[:, hold_index(keep)] on the extractor's resident int64 sums: a torch index, no kernel of the library."""
    from deep_calcium_amd import RoiTraceExtractor, hold_index
    frames, keep, rois = flashed['frames'], flashed['keep'], flashed['rois']
    ext = RoiTraceExtractor(frames.shape[1:], frames.shape[0], np.int16, rois)
    ext.feed(frames)
    sums = ext.sums_device()
    h = hold_index(keep)
    patched = sums[:, torch.from_numpy(h).to(sums.device)].cpu().numpy()
    host = sums.cpu().numpy()
    assert np.array_equal(patched, host[:, h]) and np.array_equal(patched[:, keep], host[:, keep])
    for t in flashed['idx']:
        assert np.array_equal(patched[:, t], host[:, t - 1]) and (host[:, t] > host[:, t - 1] + 1000).all()


def test_example_traces_command_drops_artefact_frames(flashed, tmp_path, monkeypatch, caplog):
    """examples/neurons/unet2ds_nf.py `traces --split --drop-artefacts [K]` on the flashed scene: the score pass logs the three
    planted frames, the split then parts the two cells it leaves as one ROI without the option, and the written traces keep every
    frame, the flashes included."""
    import importlib.util
    import logging
    import os
    from deep_calcium_amd import UNet2DSummary, hdf5_min
    frames, rois = flashed['frames'], flashed['rois']
    n_frames, h, w = frames.shape
    mask2d = np.zeros((h, w), np.float32)
    for r in rois:
        mask2d[r[:, 0], r[:, 1]] = 0.9
    path = str(tmp_path / 'scene.npz')
    np.savez(path, series_raw=frames, series_mean=frames.mean(0).astype(np.float16), name=np.array('scene'))
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'neurons', 'unet2ds_nf.py')
    state = np.random.get_state()                             # the example seeds numpy's global stream on import
    try:
        spec = importlib.util.spec_from_file_location('example_unet2ds_nf_frames', script)
        example = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(example)
    finally:
        np.random.set_state(state)
    monkeypatch.setattr(UNet2DSummary, 'predict', lambda self, dspaths, **kw: ([mask2d], ['scene']))
    for bad in (0.0, -1.0, float('nan')):
        with pytest.raises(ValueError, match='--drop-artefacts'):
            example.traces([path], None, str(tmp_path / 'no'), kind='sum', drop_artefacts=bad)
    f64 = frames.astype(np.int64)

    def rows_of(parts):
        return sorted(f64[:, p[:, 0], p[:, 1]].sum(1).tolist() for p in parts)
    whole = [rois[0], rois[1], rois[2], rois[3], rois[4]]
    parted = [rois[0], flashed['left'], flashed['right'], rois[2], rois[3], rois[4]]
    for k, want, line in ((None, whole, '0 of 5 ROIs split'), (8.0, parted, '1 of 5 ROIs split')):
        cp = str(tmp_path / ('cp%s' % k))
        caplog.clear()
        with caplog.at_level(logging.INFO, logger='traces'):
            example.traces([path], None, cp, kind='sum', split=0.1, drop_artefacts=k)
        assert line in caplog.text, caplog.text
        if k is None:
            assert 'flagged as artefacts' not in caplog.text
        else:
            assert '3 of 256 frames flagged as artefacts at K = 8' in caplog.text and ': 109 162 178' in caplog.text, caplog.text
        with hdf5_min.File(os.path.join(cp, 'scene_traces.hdf5')) as f:
            got = f['traces'].read()
        assert got.dtype == np.int64 and got.shape == (len(want), n_frames)                 # every frame, the flashes included
        assert sorted(got.tolist()) == rows_of(want)


def test_example_traces_command_scores_the_registered_frames(flashed, tmp_path, monkeypatch, caplog):
    """`traces --bidi 2 --register 2 --drop-artefacts --split --merge --bin-frames 2 --detrend 16`: the score pass runs after the
    scan-phase and the registration passes, with the registration's template, over valid_rectangle of its shifts, on the corrected
    frames (the device scores equal the oracle's on frames corrected on the host); every later pass gets the same keep, and the
    log lines count kept frames.  What the command writes is what the one-call functions give with those arguments."""
    import importlib.util
    import logging
    import os
    from deep_calcium_amd import (UNet2DSummary, estimate_bidi_device, estimate_shifts_device, extract_traces_device, flag_frames,
                                  frame_quality_device, hdf5_min, merge_rois_device, split_rois_device, valid_rectangle)
    frames, rois = flashed['frames'], flashed['rois']
    n_frames, h, w = frames.shape
    mask2d = np.zeros((h, w), np.float32)
    for r in rois:
        mask2d[r[:, 0], r[:, 1]] = 0.9
    path = str(tmp_path / 'scene.npz')
    np.savez(path, series_raw=frames, series_mean=frames.mean(0).astype(np.float16), name=np.array('scene'))
    # what the command's first passes find, and what the score pass must make of it
    off, _ = estimate_bidi_device(path, max_offset=2, frames=200)
    shifts, tmpl = estimate_shifts_device(path, max_shift=2, bidi=off)
    assert tmpl.shape == (h, w) and tmpl.dtype == frames.dtype and shifts.shape == (n_frames, 2)
    rect = valid_rectangle(shifts, (h, w), bidi=off)
    mean, corr = frame_quality_device(path, template=tmpl, rect=rect, shifts=shifts, bidi=off)
    moved = mref.apply(bref.apply(frames, off, 0), shifts, 0) if off else mref.apply(frames, shifts, 0)
    _, want_mean, want_corr = ref.scores(moved, tmpl, rect, mom=ref.moments_np)
    assert _same_bits(mean, want_mean) and _same_bits(corr, want_corr)
    keep = flag_frames(mean, corr, k=8.0)
    flagged = np.flatnonzero(~keep)
    assert set(flashed['idx'].tolist()) <= set(flagged.tolist()) and len(flagged) < 20            # the flashes, and few frames beside them
    n_kept = int(keep.sum())
    mask = mask2d.round().astype(np.uint8)
    kw = dict(shifts=shifts, bidi=off)
    b, L = 2, 16
    parts, origin, gaps = split_rois_device(path, mask, min_gap=0.1, min_area=8, bin_frames=b, detrend_frames=L, keep=keep, **kw)
    merged, morigin, pairs, mcorr = merge_rois_device(path, parts, max_dist=2, threshold=0.8, detrend_frames=L, keep=keep, **kw)
    want = extract_traces_device(path, merged, kind='sum', **kw)
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'neurons', 'unet2ds_nf.py')
    state = np.random.get_state()                             # the example seeds numpy's global stream on import
    try:
        spec = importlib.util.spec_from_file_location('example_unet2ds_nf_frames_reg', script)
        example = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(example)
    finally:
        np.random.set_state(state)
    monkeypatch.setattr(UNet2DSummary, 'predict', lambda self, dspaths, **kw: ([mask2d], ['scene']))
    cp = str(tmp_path / 'cp')
    with caplog.at_level(logging.INFO, logger='traces'):
        example.traces([path], None, cp, kind='sum', bidi=2, register=2, drop_artefacts=8.0, split=0.1, merge=0.8, bin_frames=b, detrend=L)
    text = caplog.text
    assert 'scan-phase offset %+d of the odd lines' % off in text and 'valid rectangle %r' % (rect,) in text, text
    assert '%d of %d frames flagged as artefacts at K = 8 (scored over the valid rectangle %r;' % (len(flagged), n_frames, rect) in text, text
    assert ': ' + ' '.join(str(t) for t in flagged) + '\n' in text + '\n', text
    # b and L count kept frames
    assert 'the means of %d consecutive frames: %d binned frames of %d' % (b, n_kept // b, n_kept) in text, text
    assert 'L = %d frames: %d segments over %d frames' % (L, max(1, (n_kept // b) // L), n_kept // b) in text, text
    assert '%d of %d ROIs split' % (len(parts) - len(gaps), len(gaps)) in text, text
    assert 'within segments of L = %d of all %d frames): %d candidate pairs, %d accepted, %d ROIs -> %d' % (
        L, n_kept, len(pairs), int(np.count_nonzero(mcorr >= 0.8)), len(parts), len(merged)) in text, text
    with hdf5_min.File(os.path.join(cp, 'scene_traces.hdf5')) as f:
        got = f['traces'].read()
    assert got.shape == (len(merged), n_frames) and got.dtype == want.dtype and np.array_equal(got, want)          # every frame
