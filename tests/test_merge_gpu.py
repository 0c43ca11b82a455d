"""ROI trace-pair correlation and the merge of fragmented ROIs on the device (include/dcunet.h "ROI trace-pair correlation":
dc_trace_pair_moments, dc_trace_pair_corr; merge.TracePairCorr, merge_rois_device, the example's `traces --merge`) against the
Python-integer / 60-digit decimal oracle of tests/_merge_ref.py: the six words of every pair as integers first -- with rows at the
bound, where every high word is in use --, then corr within a float32 ulp and exactly 1, -1, 0 where the header says so; the
entry points' codes; the resident sums of a streaming pass; and the bleached scene end to end, whose two distinct cells merge
without detrending and stay apart with it."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _detrend_ref as dref                       # noqa: E402
import _merge_ref as ref                          # noqa: E402
import _pair_ref as pair_ref                      # noqa: E402

R = 7
TS = (1, 2, 63, 64, 65, 257, 1000)
SEG_LENS = (0, 2, 128, 4096)
PAD = 3                                            # ld = T + 3: the words between the rows are never read
JUNK = [(-1, 0), (0, R), (2 ** 31 - 1, 0)]
PAIRS = [(0, 1), (0, 2), (2, 0), (0, 3), (3, 0), (0, 4), (4, 0), (0, 0), (1, 1), (2, 2), (2, 6), (5, 6), (6, 5), (5, 5), (6, 6), (0, 5), (4, 6),
         (0, 3), (1, 2)] + JUNK
SENTINEL = 0x5a5a5a5a5a5a5a5a


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _ulps(a, b):
    """distance in float32 steps (+0 == -0); both finite"""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def _cuda(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).cuda()


def _rows(T, L):
    """The R = 7 rows of one case, as lists of Python ints, every value inside the range |S| max(M, T) <= 2^62 of the plan:
    0 random over the whole range; 1 constant; 2 constant within every segment of the plan, stepping between them; 3 equal to row 0;
    4 the mirror image c - x of row 0; 5 and 6 AT THE BOUND, +-floor(2^62 / max(M, T)), alternating with periods 2 and 3."""
    B = 2 ** 62 // max(ref.big_m(T, L), T)
    c = 987654321
    rs = np.random.RandomState(100 * T + L)
    x = [int(rs.randint(0, 2 ** 62)) % (2 * B - c + 1) - (B - c) for _ in range(T)]          # in [c - B, B], so c - x is too
    step = [0] * T
    for s, (t0, n, _) in enumerate(ref.plan(T, L)):
        step[t0:t0 + n] = [(B // 3) * (1 - 2 * (s % 2)) - 17 * s] * n
    rows = [x, [B - 5] * T, step, list(x), [c - v for v in x], [B * (1 - 2 * (t % 2)) for t in range(T)],
            [B if t % 3 == 0 else -B for t in range(T)]]
    assert all(abs(v) <= B for r in rows for v in r)
    return rows, B


@functools.lru_cache(maxsize=None)
def _case(T, L):
    rows, B = _rows(T, L)
    moms = ref.moments(rows, PAIRS, L)
    out = dict(rows=rows, B=B, moms=moms, words=ref.moment_words(moms), corr=ref.corr(moms))
    out['words'].setflags(write=False)
    out['corr'].setflags(write=False)
    return out


def _run(dclib, rows, T, L, pairs=PAIRS, n_rows=R):
    """Both entry points by name on caller-owned buffers -> (num (P + 1, 6) int64, corr (P + 1,) float32), sentinels at P."""
    st = torch.cuda.current_stream().cuda_stream
    ld = T + PAD
    host = np.full((len(rows), ld), -SENTINEL, np.int64)                      # far outside the range: reading it would show
    host[:, :T] = np.array(rows, object).astype(np.int64) if T else 0
    sums, prs = _cuda(host, np.int64), _cuda(pairs, np.int32)
    P = len(pairs)
    num = torch.full((P + 1, 6), SENTINEL, dtype=torch.int64, device='cuda')
    corr = torch.full((P + 1,), float('nan'), dtype=torch.float32, device='cuda')
    dclib.dc_trace_pair_moments(sums.data_ptr(), ld, n_rows, T, L, prs.data_ptr(), P, num.data_ptr(), st)
    dclib.dc_trace_pair_corr(num.data_ptr(), P, corr.data_ptr(), st)
    torch.cuda.synchronize()
    return num.cpu().numpy(), corr.cpu().numpy()


# ---- 1. the raw C ABI against the oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('L', SEG_LENS)
@pytest.mark.parametrize('T', TS + (5,))
def test_moments_equal_the_oracle_word_for_word_and_corr_within_an_ulp(dclib, T, L):
    """T = 1000, L = 128: 6 x 128 and one segment of 232; T = 5, L = 2: 2 + 3; L = 2 takes the lane-per-segment path, 128 the
    wave-per-segment path, one segment the whole workgroup."""
    case = _case(T, L)
    num, corr = _run(dclib, case['rows'], T, L)
    P = len(PAIRS)
    where = dict((p, n) for n, p in enumerate(PAIRS))
    # ---- the integers ----
    assert np.array_equal(num[:P], case['words']), np.flatnonzero((num[:P] != case['words']).any(1))
    assert (num[P] == SENTINEL).all() and np.isnan(corr[P])                   # nothing at or beyond P is touched
    assert not num[P - len(JUNK):P].any() and not corr[P - len(JUNK):P].any()            # a pair that names no row: zeros, corr 0
    moms = case['moms']
    if T > 1:                                       # the rows at the bound use the high words: a 64-bit accumulator anywhere fails
        nxx = moms[where[5, 5]][0]
        assert nxx >> 64 != 0 and case['B'] ** 2 >> 64 != 0 and nxx * 4 >= ref.big_m(T, L) * T * case['B'] ** 2
        assert moms[where[5, 6]][2] >> 64 != 0
    if L and T // L <= 1:                           # L > T / 2 is one segment: the bits of seg_len = 0
        num0, corr0 = _run(dclib, case['rows'], T, 0)
        assert np.array_equal(num0, num) and np.array_equal(_bits(corr0[:P]), _bits(corr[:P]))
        assert moms == ref.moments(case['rows'], PAIRS, 0)
    # ---- corr ----
    assert np.isfinite(corr[:P]).all() and (np.abs(corr[:P]) <= 1).all()
    assert _ulps(corr[:P], case['corr']).max() <= 1, _ulps(corr[:P], case['corr'])
    for i, j in ((0, 2), (0, 3), (0, 4), (5, 6)):                             # (i, j) and (j, i): the same bits
        assert _bits(corr[where[i, j]]) == _bits(corr[where[j, i]]), (i, j)
    varies = T > 1
    assert corr[where[0, 0]] == (1 if varies else 0) and corr[where[5, 5]] == (1 if varies else 0)          # i == j on a row that varies
    assert corr[where[0, 3]] == (1 if varies else 0)                          # a row equal to another
    assert corr[where[0, 4]] == (-1 if varies else 0) and corr[where[4, 0]] == (-1 if varies else 0)        # a row against its mirror image
    for p in ((0, 1), (1, 1), (1, 2)):                                        # a constant row
        assert _bits(corr[where[p]]) == 0, p
    for p in ((0, 2), (2, 2), (2, 6)):                                        # constant within every segment of THIS plan: exactly 0
        assert _bits(corr[where[p]]) == 0 and moms[where[p]][1] == 0, p
    assert _bits(corr[P - 3]) == 0
    # two runs: identical bits
    num2, corr2 = _run(dclib, case['rows'], T, L)
    assert np.array_equal(num2, num) and np.array_equal(_bits(corr2[:P]), _bits(corr[:P]))


def test_a_row_that_steps_between_segments_is_constant_at_that_plan_only(dclib):
    """Row 2 of the T = 1000, L = 128 case is constant within each of its 7 segments: corr exactly 0 at L = 128, and an ordinary
    correlation at seg_len = 0 and at L = 96, whose segments straddle the steps."""
    T, L = 1000, 128
    rows = _case(T, L)['rows']
    pairs = [(2, 2), (0, 2), (2, 5)]
    # the rows are inside the range of L = 128, the narrowest of the three plans (its M is the largest)
    assert ref.big_m(T, L) >= ref.big_m(T, 96) and ref.big_m(T, L) >= T
    for seg, flat in ((128, True), (0, False), (96, False)):
        num, corr = _run(dclib, rows, T, seg, pairs=pairs)
        moms = ref.moments(rows, pairs, seg)
        assert np.array_equal(num[:3], ref.moment_words(moms))
        assert (moms[0][0] == 0) == flat
        if flat:
            assert not num[:3, 2:4].any() and not corr[:3].any()
        else:
            assert corr[0] == 1 and _ulps(corr[:3], ref.corr(moms)).max() <= 1 and corr[1] != 0


def test_many_pairs_of_few_frames_and_every_pair_of_rows(dclib):
    """Neither launch caps its grid (one workgroup per pair; one thread per pair): 70 000 pairs at T = 3, more than the device
    holds workgroups at once, and all R * R ordered pairs of the T = 65 case, against the oracle."""
    rs = np.random.RandomState(4)
    T, n = 3, 12
    rows = [[int(v) for v in rs.randint(-2 ** 40, 2 ** 40, size=T)] for _ in range(n)]
    every = ref.moments(rows, [(i, j) for i in range(n) for j in range(n)], 0)
    pairs = rs.randint(0, n, size=(70000, 2))
    want = ref.moment_words([every[i * n + j] for i, j in pairs.tolist()])
    num, corr = _run(dclib, rows, T, 0, pairs=pairs, n_rows=n)
    assert np.array_equal(num[:-1], want) and (num[-1] == SENTINEL).all() and np.isnan(corr[-1])
    cw = ref.corr(every)
    assert _ulps(corr[:-1], cw[pairs[:, 0] * n + pairs[:, 1]]).max() <= 1
    case = _case(65, 2)
    pairs = [(i, j) for i in range(R) for j in range(R)]
    num, corr = _run(dclib, case['rows'], 65, 2, pairs=pairs)
    moms = ref.moments(case['rows'], pairs, 2)
    assert np.array_equal(num[:-1], ref.moment_words(moms)) and _ulps(corr[:-1], ref.corr(moms)).max() <= 1
    assert np.array_equal(_bits(corr[:-1].reshape(R, R)), _bits(corr[:-1].reshape(R, R).T))


def test_entry_points_refuse_what_they_can_see_and_take_empty_sizes(dclib):
    """Every refusal of the header returns its code (-1 DC_EINVAL, -3 DC_EUNSUP) and leaves the output alone; P == 0, R == 0 and
    T == 0 return 0 and launch nothing."""
    st = torch.cuda.current_stream().cuda_stream
    T, ld, P = 8, 10, 2
    sums = _cuda(np.arange(3 * ld).reshape(3, ld), np.int64)
    pairs = _cuda([[0, 1], [1, 2]], np.int32)
    num = torch.full((P, 6), SENTINEL, dtype=torch.int64, device='cuda')
    corr = torch.full((P,), float('nan'), dtype=torch.float32, device='cuda')
    s, p, n, c = sums.data_ptr(), pairs.data_ptr(), num.data_ptr(), corr.data_ptr()
    mom, cor = dclib.cdll.dc_trace_pair_moments, dclib.cdll.dc_trace_pair_corr
    EINVAL, EUNSUP = -1, -3
    for args, code in (((None, ld, 3, T, 0, p, P, n, st), EINVAL), ((s, ld, 3, T, 0, None, P, n, st), EINVAL), ((s, ld, 3, T, 0, p, P, None, st), EINVAL),
                       ((s, ld, -1, T, 0, p, P, n, st), EINVAL), ((s, ld, 3, -1, 0, p, P, n, st), EINVAL), ((s, ld, 3, T, 0, p, -1, n, st), EINVAL),
                       ((s, T - 1, 3, T, 0, p, P, n, st), EINVAL),                                   # ld < T
                       ((s + 4, ld, 3, T, 0, p, P, n, st), EINVAL), ((s, ld, 3, T, 0, p + 2, P, n, st), EINVAL), ((s, ld, 3, T, 0, p, P, n + 4, st), EINVAL),
                       ((s, ld, 3, T, -1, p, P, n, st), EINVAL), ((s, ld, 3, T, 1, p, P, n, st), EINVAL),          # L below the range
                       ((s, ld, 3, T, 4097, p, P, n, st), EUNSUP),                                   # L above it
                       ((s, 2 ** 31, 3, 2 ** 31, 0, p, P, n, st), EUNSUP),                           # T > 2^31 - 1
                       ((s, ld, 3, T, 0, p, 2 ** 24 + 1, n, st), EUNSUP)):
        assert mom(*args) == code, args
        assert b'dc_trace_pair_moments' in dclib.cdll.dc_last_error()
    for args, code in (((None, P, c, st), EINVAL), ((n, P, None, st), EINVAL), ((n, -1, c, st), EINVAL), ((n + 4, P, c, st), EINVAL),
                       ((n, P, c + 2, st), EINVAL), ((n, 2 ** 24 + 1, c, st), EUNSUP)):
        assert cor(*args) == code, args
        assert b'dc_trace_pair_corr' in dclib.cdll.dc_last_error()
    for args in ((s, ld, 3, T, 0, p, 0, n, st), (s, ld, 0, T, 0, p, P, n, st), (s, ld, 3, 0, 0, p, P, n, st), (s, ld, 3, 0, 128, p, P, n, st)):
        assert mom(*args) == 0, args
    assert cor(n, 0, c, st) == 0
    torch.cuda.synchronize()
    assert (num.cpu().numpy() == SENTINEL).all() and np.isnan(corr.cpu().numpy()).all()              # nothing was launched
    # an 8-byte aligned column offset is the caller's pointer arithmetic; the limits themselves are accepted
    assert mom(s + 8, ld, 3, T - 1, 4096, p, P, n, st) == 0 and mom(s, ld, 3, T, 2, p, P, n, st) == 0 and cor(n, P, c, st) == 0
    torch.cuda.synchronize()
    rows = sums.cpu().numpy()[:, :T].tolist()
    assert np.array_equal(num.cpu().numpy(), ref.moment_words(ref.moments(rows, [(0, 1), (1, 2)], 2)))


# ---- 2. TracePairCorr on the resident sums of a streaming pass -------------------------------------------------------------------------
def _halves(region, gap=0):
    """The left and the right half of a 6 x 12 region; gap = 1 leaves the column between them out (two fragments one blank pixel apart)."""
    x0 = int(region[:, 1].min())
    return region[region[:, 1] < x0 + 6 - gap], region[region[:, 1] >= x0 + 6]


@functools.lru_cache(maxsize=None)
def _scene(beta=None, gap=0, strip=True):
    """_pair_ref.gpu_scene(): the regions static, two, same, gauss, each as two ROIs, and the strip -> frames, ROIs, their int sums."""
    frames, rois, _, _ = pair_ref.gpu_scene()
    if beta is not None:
        frames = dref.bleach(frames, beta)
    frames.setflags(write=False)
    out = []
    for r in (rois[0], rois[1], rois[3], rois[4]):
        out += list(_halves(r, gap))
    if strip:
        out.append(rois[2])
    f = frames.astype(np.int64)
    sums = [f[:, r[:, 0], r[:, 1]].sum(1).tolist() for r in out]
    return frames, out, sums


@pytest.mark.parametrize('L', [None, 64])
def test_trace_pair_corr_on_the_resident_sums_of_an_extractor(L):
    """The sums stay where RoiTraceExtractor left them (ragged chunks of 100, 100, 56 frames): moments equal the oracle's, corr
    within an ulp, and merge_rois of the device's corr is the oracle's merge -- which joins the halves of 'same' (ROIs 4, 5) and
    leaves the two cells of 'two' (ROIs 2, 3) apart."""
    from deep_calcium_amd import RoiTraceExtractor, TracePairCorr, merge_rois, roi_neighbours
    frames, rois, sums = _scene()
    shape = frames.shape[1:]
    pairs = roi_neighbours(rois, shape, max_dist=2)
    assert pairs.tolist() == [list(p) for p in ref.neighbours([r.tolist() for r in rois], 2)]
    assert [0, 1] in pairs.tolist() and [2, 3] in pairs.tolist() and [4, 5] in pairs.tolist() and [6, 7] in pairs.tolist() and len(pairs) > 4
    ext = RoiTraceExtractor(shape, frames.shape[0], frames.dtype, rois, chunk_frames=100)
    for t0 in range(0, frames.shape[0], 100):
        ext.feed(frames[t0:t0 + 100])
    resident = ext.sums_device()
    tp = TracePairCorr(resident, ext.areas_host(), pairs, detrend_frames=L)
    assert tp._src.data_ptr() == resident.data_ptr()                          # read in place
    moms = ref.moments(sums, pairs.tolist(), L)
    M = ref.big_m(frames.shape[0], L)
    assert tp.result('moments') == [dict(Nxx=a, Nxy=b, Nyy=c, M=M) for a, b, c in moms]
    corr = tp.result('corr')
    want = ref.corr(moms)
    assert corr.dtype == np.float32 and corr.shape == (len(pairs),) and _ulps(corr, want).max() <= 1
    assert np.array_equal(tp.pairs(), pairs)
    # numpy sums give the same bits as resident ones
    again = TracePairCorr(np.array(sums, np.int64), ext.areas_host(), pairs, detrend_frames=L)
    assert np.array_equal(_bits(again.result('corr')), _bits(corr)) and again.result('moments') == tp.result('moments')
    new, origin = merge_rois(rois, pairs, corr, shape, threshold=0.8)
    wnew, worigin = ref.merge([r.tolist() for r in rois], pairs.tolist(), want.tolist(), shape[1], 0.8)
    assert origin == worigin and [n.tolist() for n in new] == [[list(p) for p in w] for w in wnew]
    assert [4, 5] in origin and [2] in origin and [3] in origin
    c64 = dict(zip(map(tuple, pairs.tolist()), ref.corr64(moms)))
    assert c64[4, 5] >= 0.9 and c64[2, 3] <= 0.5                              # far from the threshold: an ulp decides nothing


# ---- 3. the bleached scene, end to end ---------------------------------------------------------------------------------------------------
def _oracle_merge(sums, rois, pairs, L, W):
    moms = ref.moments(sums, pairs, L)
    return ref.merge([r.tolist() for r in rois], pairs, ref.corr(moms).tolist(), W, 0.8), ref.corr64(moms)


def test_the_bleached_scene_merges_distinct_cells_unless_detrended(tmp_path, monkeypatch):
    """_pair_ref.gpu_scene() bleached to half its brightness, the halves of every region as two ROIs: the whole-recording
    correlation merges the two distinct cells of 'two' (ROIs 2, 3); pooled over segments of 128 frames it does not, and still merges
    the halves of 'same' (ROIs 4, 5).  With no candidate pair the recording is not read."""
    from deep_calcium_amd import merge_rois_device
    frames, rois, sums = _scene(beta=0.5, strip=False)
    W = frames.shape[2]
    path = str(tmp_path / 'bleached.npz')
    np.savez(path, series_raw=frames)
    cand = [(0, 1), (2, 3), (4, 5), (6, 7)]
    for L, two_merges in ((None, True), (128, False)):
        (wnew, worigin), c64 = _oracle_merge(sums, rois, cand, L, W)
        assert (c64[1] >= 0.85) if two_merges else (c64[1] <= 0.75), c64
        assert c64[2] >= 0.9
        new, origin, pairs, corr = merge_rois_device(path, rois, detrend_frames=L, chunk_frames=100)
        assert pairs.tolist() == [list(p) for p in cand] and pairs.dtype == np.int32 and corr.dtype == np.float32
        assert _ulps(corr, ref.corr(ref.moments(sums, cand, L))).max() <= 1
        assert origin == worigin and [n.tolist() for n in new] == [[list(p) for p in w] for w in wnew]
        assert ([2, 3] in origin) == two_merges and [4, 5] in origin
    # ROIs that are all apart: no candidates, no extractor, no pass over the recording
    import deep_calcium_amd.traces

    def no_pass(*a, **k):
        raise AssertionError('the recording is read although there is no candidate pair')
    monkeypatch.setattr(deep_calcium_amd.traces, 'RoiTraceExtractor', no_pass)
    apart = [rois[0], rois[2]]
    new, origin, pairs, corr = merge_rois_device(path, apart, max_dist=2, source='series/raw')
    assert origin == [[0], [1]] and pairs.shape == (0, 2) and corr.shape == (0,) and [n.tolist() for n in new] == [r.tolist() for r in apart]


def test_example_traces_command_merges_fragments(tmp_path, monkeypatch, caplog):
    """examples/neurons/unet2ds_nf.py `traces --merge [THR] [--detrend L]` on the bleached scene, every region delivered by the mask as
    two fragments one blank column apart: --merge alone joins all four pairs, the two distinct cells included; with --detrend 128
    the two cells stay two ROIs and the other three regions are joined.  The log lines name the counts; --detrend alone is still
    refused in the old words."""
    import importlib.util
    import logging
    import os
    from deep_calcium_amd import UNet2DSummary, hdf5_min
    frames, rois, sums = _scene(beta=0.5, gap=1, strip=False)
    n_frames, h, w = frames.shape
    (_, worigin), c64 = _oracle_merge(sums, rois, [(0, 1), (2, 3), (4, 5), (6, 7)], None, w)
    (_, dorigin), d64 = _oracle_merge(sums, rois, [(0, 1), (2, 3), (4, 5), (6, 7)], 128, w)
    assert worigin == [[0, 1], [2, 3], [4, 5], [6, 7]] and c64.min() >= 0.85
    assert dorigin == [[0, 1], [2], [3], [4, 5], [6, 7]] and d64[1] <= 0.75 and np.delete(d64, 1).min() >= 0.9
    mask2d = np.zeros((h, w), np.float32)
    for r in rois:
        mask2d[r[:, 0], r[:, 1]] = 0.9
    path = str(tmp_path / 'scene.npz')
    np.savez(path, series_raw=frames, series_mean=frames.mean(0).astype(np.float16), name=np.array('scene'))
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'neurons', 'unet2ds_nf.py')
    state = np.random.get_state()                             # the example seeds numpy's global stream on import
    try:
        spec = importlib.util.spec_from_file_location('example_unet2ds_nf_merge', script)
        example = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(example)
    finally:
        np.random.set_state(state)
    monkeypatch.setattr(UNet2DSummary, 'predict', lambda self, dspaths, **kw: ([mask2d], ['scene']))
    with pytest.raises(ValueError, match='--detrend needs --refine or --split'):
        example.traces([path], None, str(tmp_path / 'no'), kind='sum', detrend=64)
    with pytest.raises(ValueError, match='--merge-dist'):
        example.traces([path], None, str(tmp_path / 'no'), kind='sum', merge=0.8, merge_dist=17)
    with pytest.raises(ValueError, match='--merge joins'):
        example.traces([path], None, str(tmp_path / 'no'), kind='sum', merge=float('nan'))
    f64 = frames.astype(np.int64)
    for detrend, want, line in ((None, worigin, '4 candidate pairs, 4 accepted, 8 ROIs -> 4'), (128, dorigin, '4 candidate pairs, 3 accepted, 8 ROIs -> 5')):
        cp = str(tmp_path / ('cp%s' % detrend))
        caplog.clear()
        with caplog.at_level(logging.INFO, logger='traces'):
            example.traces([path], None, cp, kind='sum', merge=0.8, merge_dist=2, detrend=detrend)
        assert 'merged at trace corr >= 0.8 (within 2 pixels' in caplog.text and line in caplog.text, caplog.text
        if detrend is not None:
            assert 'L = 128 frames: 2 segments over 256 frames, L_last = 128' in caplog.text          # the existing line, word for word
        with hdf5_min.File(os.path.join(cp, 'scene_traces.hdf5')) as f:
            got = f['traces'].read()
        assert got.dtype == np.int64 and got.shape == (len(want), n_frames)
        for row, members in zip(got, want):
            pix = np.concatenate([rois[m] for m in members])
            assert np.array_equal(row, f64[:, pix[:, 0], pix[:, 1]].sum(1)), members
    # at distance 1 the fragments, one blank column apart, are no candidates: nothing is merged and the pass is not made
    caplog.clear()
    with caplog.at_level(logging.INFO, logger='traces'):
        example.traces([path], None, str(tmp_path / 'cp1'), kind='sum', merge=0.8, merge_dist=1)
    assert '0 candidate pairs, 0 accepted, 8 ROIs -> 8' in caplog.text
