"""Detrended (segment-pooled) correlations on the device (include/dcunet.h "Detrended correlations": dc_series_fold_segment,
dc_series_finalize_pooled, dc_roi_pair_fold_segment, dc_roi_pair_corr_pooled, dc_roi_pixel_fold_segment,
dc_roi_pixel_corr_pooled; `detrend_frames=` of the three readers) against the Python-integer / 60-digit decimal oracle of
tests/_detrend_ref.py: the pooled numerators as integers first, then corr bit for bit, for every chunking; one segment against the
undetrended readers; binning in front; and the split of the bleached scene whose conditions tests/test_detrend_api.py checks on
the oracle."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _detrend_ref as ref                        # noqa: E402
import _pair_ref as pair_ref                      # noqa: E402
import _tbin_ref as tbin_ref                      # noqa: E402
from test_series_gpu import _frames, _ulps        # noqa: E402  the full-range frames (extremes held and alternating) and the float32 distance

T_SERIES, L_SERIES = 37, 8                        # segments of 8, 8, 8 and 13 frames


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def _feed(reader, frames, chunk):
    for t0 in range(0, frames.shape[0], chunk):
        reader.feed(frames[t0:t0 + chunk])
    return reader


# ---- 1. the series image ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _series_oracle(H, W, dtype):
    frames = _frames(T_SERIES, H, W, np.dtype(dtype).type)
    var, cov = ref.series_numerators(frames, L_SERIES)
    M = ref.big_m(T_SERIES, L_SERIES)
    out = dict(frames=frames, var=var, cov=cov, M=M, corr=ref.series_corr(var, cov), std=ref.series_std(var, M, T_SERIES))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@pytest.mark.parametrize('dtype', ['int16', 'uint16'])
@pytest.mark.parametrize('shape', [(5, 7), (9, 70)])        # 35 pixels; a row wider than one wave and more than one workgroup
def test_series_numerators_corr_and_std_equal_the_oracle(shape, dtype):
    from deep_calcium_amd import SeriesSummarizer
    H, W = shape
    want = _series_oracle(H, W, dtype)
    frames = want['frames']
    assert want['M'] == 8 * 13 and frames[:, 0, 0].min() == np.iinfo(frames.dtype).min      # the extremes are in
    kinds = ('mean', 'max', 'std', 'corr')
    plain = _feed(SeriesSummarizer(shape, T_SERIES, frames.dtype, kinds=kinds), frames, T_SERIES)
    first = None
    for chunk in (T_SERIES, 1, 5):                          # whole; every frame a chunk; boundaries inside segments
        summ = _feed(SeriesSummarizer(shape, T_SERIES, frames.dtype, kinds=kinds, chunk_frames=chunk, detrend_frames=L_SERIES), frames, chunk)
        mom = summ.result('moments')
        assert mom['M'] == want['M'] and mom['T'] == T_SERIES
        assert np.array_equal(mom['var'], want['var']) and np.array_equal(mom['cov'], want['cov']), chunk      # integers first
        got = dict((k, summ.result(k)) for k in kinds)
        assert np.array_equal(_bits(got['corr']), _bits(want['corr'])), (chunk, _ulps(got['corr'], want['corr']).max())
        assert _ulps(got['std'], want['std']).max() <= 1, chunk
        for k in ('mean', 'max'):                           # the whole recording's, as without the keyword
            assert np.array_equal(_bits(got[k]), _bits(plain.result(k))), (chunk, k)
        if first is None:
            first = got
        for k in kinds:
            assert np.array_equal(_bits(got[k]), _bits(first[k])), (chunk, k)
    assert (want['var'] == 0).any() and (np.abs(want['corr']) > 0).any()
    # one segment (L > T / 2): the corr bits of the undetrended reader, std within 1 ulp
    one = _feed(SeriesSummarizer(shape, T_SERIES, frames.dtype, kinds=kinds, chunk_frames=5, detrend_frames=19), frames, 5)
    assert np.array_equal(_bits(one.result('corr')), _bits(plain.result('corr')))
    assert _ulps(one.result('std'), plain.result('std')).max() <= 1
    assert one.result('moments')['M'] == T_SERIES
    # without 'corr' there is no pair state at all
    sd = _feed(SeriesSummarizer(shape, T_SERIES, frames.dtype, kinds=('std',), chunk_frames=5, detrend_frames=L_SERIES), frames, 5)
    assert np.array_equal(_bits(sd.result('std')), _bits(first['std'])) and sd.result('moments')['cov'] is None


def test_series_one_call_function_and_binning_in_front(tmp_path):
    from deep_calcium_amd import summarize_series_device
    frames = _frames(T_SERIES * 2 + 1, 5, 7, np.int16, seed=1)
    path = str(tmp_path / 'rec.npz')
    np.savez(path, series_raw=frames)
    binned = tbin_ref.bin_time(frames, 2)                                      # 37 bins; the last frame closes none
    var, cov = ref.series_numerators(binned, L_SERIES)
    got = summarize_series_device(path, kind='corr', standardize=False, chunk_frames=5, bin_frames=2, detrend_frames=L_SERIES)
    assert np.array_equal(_bits(got), _bits(ref.series_corr(var, cov)))
    var, cov = ref.series_numerators(frames, L_SERIES)
    got = summarize_series_device(path, kind='std', standardize=False, chunk_frames=7, detrend_frames=L_SERIES)
    assert _ulps(got, ref.series_std(var, ref.big_m(frames.shape[0], L_SERIES), frames.shape[0])).max() <= 1


# ---- 2. pairs and footprints on the scene ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scene():
    frames, rois, left, right = pair_ref.gpu_scene()
    frames.setflags(write=False)
    return frames, rois, left, right


@functools.lru_cache(maxsize=None)
def _pair_oracle(L, bin_frames=1):
    frames, rois, _, _ = _scene()
    if bin_frames > 1:
        frames = tbin_ref.bin_time(frames, bin_frames)
    N = [ref.pooled_gram(frames[:, r[:, 0], r[:, 1]], L) for r in rois]
    return N, [ref.pair_corr(n) for n in N], ref.big_m(frames.shape[0], L)


def _check_pairs(pc, L, bin_frames=1):
    N, corr, M = _pair_oracle(L, bin_frames)
    mom = pc.result('moments')
    for r in range(len(N)):
        assert mom[r]['M'] == M and np.array_equal(mom[r]['N'], N[r]), r                  # integers first
    got = pc.result('corr')
    for r in range(len(N)):
        assert np.array_equal(_bits(got[r]), _bits(corr[r])), (r, _ulps(got[r], corr[r]).max())
        assert np.array_equal(_bits(got[r]), _bits(got[r].T)) and (np.diag(got[r]) == 1).all()
    return got


@pytest.mark.parametrize('L', [64, 100])                    # four segments of 64; segments of 100 and 156 frames
def test_pair_numerators_and_corr_equal_the_oracle(L):
    from deep_calcium_amd import RoiPairCorr
    frames, rois, _, _ = _scene()
    T, h, w = frames.shape
    assert len(rois[1]) == 72 and T == 256                  # 72 pixels: tiles (0,0), (0,1), (1,1)
    first = None
    for chunk in (256, 37, 1):
        pc = _feed(RoiPairCorr((h, w), T, frames.dtype, rois, chunk_frames=chunk, detrend_frames=L), frames, chunk)
        got = _check_pairs(pc, L)
        first = first or got
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(got, first)), chunk
        if chunk == 37:                                     # the traces of the same pass are the recording's, not detrended
            assert np.array_equal(pc.traces('sum')[1], frames[:, rois[1][:, 0], rois[1][:, 1]].astype(np.int64).sum(1))


def test_pairs_of_an_roi_wider_than_a_workgroup():
    """An ROI of 300 pixels: 15 tiles with ragged last ones, and rows of the matrix longer than the 256 lanes that write them."""
    from deep_calcium_amd import RoiPairCorr
    rs = np.random.RandomState(21)
    T, h, w, L = 12, 10, 40, 5                                                 # segments of 5 and 7 frames
    frames = rs.randint(0, 4096, size=(T, h, w)).astype(np.uint16)
    flat = np.sort(rs.choice(h * w, 300, replace=False))
    roi = np.stack([flat // w, flat % w], 1)
    pc = _feed(RoiPairCorr((h, w), T, frames.dtype, [roi], chunk_frames=4, detrend_frames=L), frames, 4)
    assert pc.n_tiles == 15
    N = ref.pooled_gram(frames.reshape(T, -1)[:, flat], L)
    mom = pc.result('moments')[0]
    assert mom['M'] == 35 and np.array_equal(mom['N'], N)
    got = pc.result('corr')[0]
    assert np.array_equal(_bits(got), _bits(got.T)) and (np.diag(got) == 1).all()
    for i in (0, 63, 64, 255, 256, 299):                                       # whole rows, columns beyond 256 included
        want = np.array([ref.corr_exact(N[i][i], N[i][j], N[j][j]) for j in range(300)], np.float32)
        assert np.array_equal(_bits(got[i]), _bits(want)), (i, _ulps(got[i], want).max())


def test_pairs_one_segment_is_the_undetrended_reader_and_binning_comes_first(tmp_path):
    from deep_calcium_amd import RoiPairCorr, roi_pair_corr_device
    frames, rois, _, _ = _scene()
    T, h, w = frames.shape
    plain = _feed(RoiPairCorr((h, w), T, frames.dtype, rois, chunk_frames=37), frames, 37).result('corr')
    one = _feed(RoiPairCorr((h, w), T, frames.dtype, rois, chunk_frames=37, detrend_frames=200), frames, 37)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(one.result('corr'), plain))
    assert one.result('moments')[0]['M'] == T
    path = str(tmp_path / 'scene.npz')
    np.savez(path, series_raw=frames)
    corr, pixels = roi_pair_corr_device(path, rois, chunk_frames=37, bin_frames=2, detrend_frames=32)      # 128 bins: four segments of 32
    want = _pair_oracle(32, 2)[1]
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(corr, want))
    assert all(np.array_equal(p, r) for p, r in zip(pixels, rois))


@functools.lru_cache(maxsize=None)
def _footprint_oracle(L, bin_frames=1):
    from deep_calcium_amd import roi_support
    frames, rois, _, _ = _scene()
    if bin_frames > 1:
        frames = tbin_ref.bin_time(frames, bin_frames)
    W = frames.shape[2]
    coords, inside = roi_support(rois, frames.shape[1:], halo=2)
    nums, corr = [], []
    for r, c, ins in zip(rois, coords, inside):
        n = ref.footprint_numerators(frames, (r[:, 0] * W + r[:, 1]).tolist(), (c[:, 0] * W + c[:, 1]).tolist(), L)
        nums.append(n)
        corr.append(ref.footprint_corr(n[0], n[1], n[2], ins))
    return nums, corr, ref.big_m(frames.shape[0], L)


def _check_footprints(fp, L, bin_frames=1):
    nums, corr, M = _footprint_oracle(L, bin_frames)
    mom = fp.result('moments')
    for r, (cxx, cxs, css) in enumerate(nums):
        assert mom[r]['M'] == M and mom[r]['Css'] == css and mom[r]['Cxx'].tolist() == cxx and mom[r]['Cxs'].tolist() == cxs, r
    got = fp.result('corr')
    for r in range(len(nums)):
        assert np.array_equal(_bits(got[r]), _bits(corr[r])), (r, _ulps(got[r], corr[r]).max())
    return got


@pytest.mark.parametrize('L', [64, 100])
def test_footprint_numerators_and_corr_equal_the_oracle(L):
    from deep_calcium_amd import RoiFootprints
    frames, rois, _, _ = _scene()
    T, h, w = frames.shape
    first = None
    for chunk in (256, 37, 1):
        fp = _feed(RoiFootprints((h, w), T, frames.dtype, rois, halo=2, chunk_frames=chunk, detrend_frames=L), frames, chunk)
        got = _check_footprints(fp, L)
        first = first or got
        assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(got, first)), chunk
    assert any(i.any() and not i.all() for i in fp.inside())                               # inside and halo entries both
    assert np.array_equal(fp.traces('sum')[1], frames[:, rois[1][:, 0], rois[1][:, 1]].astype(np.int64).sum(1))


def test_footprints_one_segment_is_the_undetrended_reader_and_binning_comes_first(tmp_path):
    from deep_calcium_amd import RoiFootprints, roi_footprints_device
    frames, rois, _, _ = _scene()
    T, h, w = frames.shape
    plain = _feed(RoiFootprints((h, w), T, frames.dtype, rois, halo=2, chunk_frames=37), frames, 37).result('corr')
    one = _feed(RoiFootprints((h, w), T, frames.dtype, rois, halo=2, chunk_frames=37, detrend_frames=200), frames, 37)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(one.result('corr'), plain))
    path = str(tmp_path / 'scene.npz')
    np.savez(path, series_raw=frames)
    corr, coords, inside = roi_footprints_device(path, rois, halo=2, chunk_frames=37, bin_frames=2, detrend_frames=32)
    want = _footprint_oracle(32, 2)[1]
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(corr, want))


# ---- 3. the raw C ABI: what the readers never do -----------------------------------------------------------------------------------
def _cuda(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).cuda()


def _words(t):
    """int64 (n, 2) {lo, hi} on the device -> Python ints."""
    w = t.cpu().numpy()
    return [int(hi) * (1 << 64) + int(np.uint64(lo)) for lo, hi in w.reshape(-1, 2)]


def test_pixel_fold_walks_a_row_longer_than_a_workgroup_and_skips_unnamed_rows(dclib):
    """dc_roi_pixel_fold_segment / dc_roi_pixel_corr_pooled on caller-owned buffers: a CSR row of 600 entries (the lanes of a
    workgroup loop over it), a row that names no ROI (left alone, corr 0), pre-loaded pooled words (the fold ADDS), mom cleared
    for the folded rows only, and the words beyond the state untouched."""
    L = dclib
    st = torch.cuda.current_stream().cuda_stream
    rs = np.random.RandomState(11)
    N, R, n, mult = 600 + 5 + 3, 2, 13, 8
    row_off, row_roi = [0, 600, 605, 608], [1, 7, 0]                           # row 1 names ROI 7 of 2: skipped
    a = rs.randint(-32768 * n, 65535 * n, size=N)
    b = rs.randint(0, 65535 ** 2 * n, size=N)
    c = [int(v) * int(s) for v, s in zip(rs.randint(-2 ** 40, 2 ** 40, size=N), rs.randint(1, 2 ** 30, size=N))]      # beyond 64 bits
    u = [int(rs.randint(-2 ** 40, 2 ** 40)) for _ in range(R)]
    w = [x * x + int(rs.randint(0, 2 ** 60)) * 2 ** 20 for x in u]
    mom = np.stack([a, b, np.array([v & (2 ** 64 - 1) for v in c], np.uint64).view(np.int64), np.array([v >> 64 for v in c], np.int64)])
    rmom = np.stack([np.array(u, np.int64), np.array([v & (2 ** 64 - 1) for v in w], np.uint64).view(np.int64), np.array([v >> 64 for v in w], np.int64)])
    d_mom, d_rmom = _cuda(mom, np.int64), _cuda(rmom, np.int64)
    d_off, d_roi = _cuda(row_off, np.int32), _cuda(row_roi, np.int32)
    pre = (1 << 100) + 12345                                                   # what every pooled word holds before: the fold adds
    word = [pre & (2 ** 64 - 1), (pre >> 64) & (2 ** 64 - 1)]
    fill = lambda k: _cuda(np.array([word] * k + [[0x5a5a, 0x5a5a]], np.uint64).view(np.int64), np.int64)      # noqa: E731
    pxx, pxs, pss = fill(N), fill(N), fill(R)
    L.dc_roi_pixel_fold_segment(d_mom.data_ptr(), N, d_off.data_ptr(), d_roi.data_ptr(), 3, R, d_rmom.data_ptr(), n, mult,
                                pxx.data_ptr(), pxs.data_ptr(), pss.data_ptr(), 5, 7, st)
    torch.cuda.synchronize()
    gxx, gxs, gss = _words(pxx), _words(pxs), _words(pss)
    named = [1] * 600 + [None] * 5 + [0] * 3
    for e in range(N):
        r = named[e]
        wxx = pre + (0 if r is None else mult * (n * int(b[e]) - int(a[e]) ** 2))
        wxs = pre + (0 if r is None else mult * (n * c[e] - int(a[e]) * u[r]))
        assert gxx[e] == wxx and gxs[e] == wxs, e
    for r in range(R):
        assert gss[r] == pre + mult * (n * w[r] - u[r] * u[r]), r
    sentinel = 0x5a5a * (1 << 64) + 0x5a5a
    assert gxx[N] == gxs[N] == gss[R] == sentinel                              # nothing beyond the state
    after = d_mom.cpu().numpy()
    assert not after[:, :600].any() and not after[:, 605:].any() and np.array_equal(after[:, 600:605], mom[:, 600:605])
    inside = _cuda(rs.randint(0, 2, size=N), np.int32)
    corr = torch.full((N + 1,), float('nan'), dtype=torch.float32, device='cuda')
    L.dc_roi_pixel_corr_pooled(pxx.data_ptr(), pxs.data_ptr(), pss.data_ptr(), N, d_off.data_ptr(), d_roi.data_ptr(), 3, R,
                               inside.data_ptr(), corr.data_ptr(), st)
    torch.cuda.synchronize()
    corr = corr.cpu().numpy()
    assert np.isnan(corr[N]) and np.isfinite(corr[:N]).all() and not corr[600:605].any()      # the unnamed row: 0
    flags = inside.cpu().numpy() != 0
    for lo, hi, r in ((0, 600, 1), (605, 608, 0)):                             # the rule on whatever integers the words hold
        want = ref.footprint_corr(gxx[lo:hi], gxs[lo:hi], gss[r], flags[lo:hi])
        assert np.array_equal(_bits(corr[lo:hi]), _bits(want)), (r, _ulps(corr[lo:hi], want).max())


def test_the_fold_entry_points_on_caller_owned_buffers(dclib):
    """dc_series_fold_segment, dc_series_finalize_pooled, dc_roi_pair_fold_segment, dc_roi_pair_corr_pooled by name: two segments
    of 5 and 7 frames (mult 7 and 5) of a 3 x 6 recording fed through the undetrended accumulate entry points, the pooled words
    against the oracle's integers; the pair fold leaves a and g zero and the lower triangle alone."""
    L = dclib
    st = torch.cuda.current_stream().cuda_stream
    H, W, T, seg = 3, 6, 12, 5
    frames = _frames(T, H, W, np.int16, seed=2)
    plan = ref.plan(T, seg)
    assert plan == [(0, 5, 7), (5, 7, 5)]
    d = _cuda(frames, np.int16)
    n = H * W
    z64 = lambda *s: torch.zeros(s, dtype=torch.int64, device='cuda')          # noqa: E731
    s1, s2, xy, vm = z64(n), z64(n), z64(4, n), torch.zeros(n, dtype=torch.int32, device='cuda')
    pvar, pcov, tot = z64(n, 2), z64(4, n, 2), z64(n)
    vt = torch.full((n,), -2 ** 31, dtype=torch.int32, device='cuda')
    # pairs: one ROI of all 18 pixels
    off, pix, goff, tiles = _cuda([0, n], np.int32), _cuda(np.arange(n), np.int32), _cuda([0], np.int64), _cuda([[0, 0, 0]], np.int32)
    a, g, pooled = z64(n), z64(n * n), z64(n * n + 1, 2)
    pooled[n * n] = 0x5a5a
    for t0, length, mult in plan:
        fp = d[t0:t0 + length].data_ptr()
        L.dc_series_accumulate(fp, 0, length, 0, length, None, None, s1.data_ptr(), s2.data_ptr(), vm.data_ptr(), H, W, st)
        L.dc_series_accumulate_xy(fp, 0, length, 0, xy.data_ptr(), H, W, st)
        L.dc_series_fold_segment(s1.data_ptr(), s2.data_ptr(), xy.data_ptr(), vm.data_ptr(), length, mult, pvar.data_ptr(), pcov.data_ptr(),
                                 tot.data_ptr(), vt.data_ptr(), H, W, st)
        L.dc_roi_pair_accumulate(fp, 0, length, off.data_ptr(), pix.data_ptr(), goff.data_ptr(), tiles.data_ptr(), 1, 1, a.data_ptr(),
                                 g.data_ptr(), n, n * n, H, W, st)
        L.dc_roi_pair_fold_segment(a.data_ptr(), g.data_ptr(), off.data_ptr(), goff.data_ptr(), tiles.data_ptr(), 1, 1, n, n * n, length, mult,
                                   pooled.data_ptr(), st)
        torch.cuda.synchronize()
        assert not a.cpu().numpy().any() and not g.cpu().numpy().any()         # left zero for the next segment
    var, cov = ref.series_numerators(frames, seg)
    assert _words(pvar) == var.ravel().tolist() and _words(pcov) == cov.ravel().tolist()
    assert np.array_equal(tot.cpu().numpy(), frames.astype(np.int64).sum(0).ravel()) and np.array_equal(vt.cpu().numpy(), frames.max(0).ravel())
    N = ref.pooled_gram(frames.reshape(T, n), seg)
    got = np.array(_words(pooled), object)
    assert got[n * n] == 0x5a5a * (1 << 64) + 0x5a5a
    assert np.array_equal(got[:n * n].reshape(n, n), np.triu(N))              # the lower triangle is never touched
    out = torch.full((3, n), float('nan'), dtype=torch.float32, device='cuda')
    L.dc_series_finalize_pooled(pvar.data_ptr(), pcov.data_ptr(), tot.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), H, W,
                                35, T, st)
    corr = torch.full((n * n + 1,), float('nan'), dtype=torch.float32, device='cuda')
    L.dc_roi_pair_corr_pooled(pooled.data_ptr(), off.data_ptr(), goff.data_ptr(), 1, n, n * n, corr.data_ptr(), st)
    torch.cuda.synchronize()
    out, corr = out.cpu().numpy(), corr.cpu().numpy()
    assert np.array_equal(_bits(out[2].reshape(H, W)), _bits(ref.series_corr(var, cov)))
    assert _ulps(out[1].reshape(H, W), ref.series_std(var, 35, T)).max() <= 1
    assert np.array_equal(_bits(out[0]), _bits((frames.astype(np.int64).sum(0).ravel() / np.float64(T)).astype(np.float32)))
    assert np.isnan(corr[n * n]) and np.array_equal(_bits(corr[:n * n].reshape(n, n)), _bits(ref.pair_corr(N)))


# ---- 4. the bleached scene, end to end ---------------------------------------------------------------------------------------------
def test_the_bleached_scene_is_split_only_when_detrended(tmp_path):
    """_pair_ref.gpu_scene() bleached to half its brightness (tests/test_detrend_api.py checks both outcomes on the oracle for
    this seed, beta = 0.5 and L = 64, with margins far above a float32 ulp): the whole-recording correlation leaves the two-cell
    region whole, segments of 64 frames split it into the planted halves; the controls and the strip stay as they are."""
    from deep_calcium_amd import split_rois_device
    frames, rois, left, right = _scene()
    frames = ref.bleach(frames, 0.5)
    path = str(tmp_path / 'bleached.npz')
    np.savez(path, series_raw=frames)
    new, origin, gaps = split_rois_device(path, rois, min_gap=0.1, min_area=8, iterations=16, chunk_frames=100)
    assert origin == [0, 1, 2, 3, 4] and gaps[1] < 0.08 and all(np.array_equal(x, y) for x, y in zip(new, rois))
    new, origin, gaps = split_rois_device(path, rois, min_gap=0.1, min_area=8, iterations=16, chunk_frames=100, detrend_frames=64)
    assert origin == [0, 1, 1, 2, 3, 4] and len(new) == 6
    assert np.array_equal(new[1], left) and np.array_equal(new[2], right)       # 0 pixels misassigned, none dropped
    for n, r in ((0, 0), (3, 2), (4, 3), (5, 4)):
        assert np.array_equal(new[n], rois[r])                                  # static, strip, same, gauss: unchanged in both modes
    assert gaps[1] >= 0.15 and np.isnan(gaps[2]) and all(not g >= 0.05 for g in gaps[[0, 3, 4]])


def test_example_traces_command_detrends_the_split(tmp_path, monkeypatch, caplog):
    """examples/neurons/unet2ds_nf.py `traces --split GAP --detrend L`: the bleached scene is split only with the flag, which
    logs L, the number of segments and L_last; the traces that are written are those of every frame, not detrended."""
    import importlib.util
    import logging
    import os
    from deep_calcium_amd import UNet2DSummary, hdf5_min
    frames, rois, left, right = _scene()
    frames = ref.bleach(frames, 0.5)
    n_frames, h, w = frames.shape
    mask2d = np.zeros((h, w), np.float32)
    for r in rois:
        mask2d[r[:, 0], r[:, 1]] = 0.9
    path = str(tmp_path / 'scene.npz')
    np.savez(path, series_raw=frames, series_mean=frames.mean(0).astype(np.float16), name=np.array('scene'))
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'neurons', 'unet2ds_nf.py')
    state = np.random.get_state()                             # the example seeds numpy's global stream on import
    try:
        spec = importlib.util.spec_from_file_location('example_unet2ds_nf_detrend', script)
        example = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(example)
    finally:
        np.random.set_state(state)
    monkeypatch.setattr(UNet2DSummary, 'predict', lambda self, dspaths, **kw: ([mask2d], ['scene']))
    with pytest.raises(ValueError, match='--detrend needs --refine or --split'):
        example.traces([path], None, str(tmp_path / 'no'), kind='sum', detrend=64)
    with pytest.raises(ValueError, match=r'L in \[2, 4096\]'):
        example.traces([path], None, str(tmp_path / 'no'), kind='sum', split=0.1, detrend=1)
    cp = str(tmp_path / 'cp')
    with caplog.at_level(logging.INFO, logger='traces'):
        example.traces([path], None, cp, kind='sum', split=0.1, min_area=8, detrend=100)
    assert 'L = 100 frames: 2 segments over 256 frames, L_last = 156' in caplog.text
    assert '1 of 5 ROIs split, 0 pixels dropped' in caplog.text
    with hdf5_min.File(os.path.join(cp, 'scene_traces.hdf5')) as f:
        got = f['traces'].read()
    # the mask's regions in raster label order: the strip (row 0), then the four regions left to right
    assert got.dtype == np.int64 and got.shape == (6, n_frames)
    assert np.array_equal(got[2], frames[:, left[:, 0], left[:, 1]].astype(np.int64).sum(1))
    assert np.array_equal(got[3], frames[:, right[:, 0], right[:, 1]].astype(np.int64).sum(1))
    caplog.clear()
    cp2 = str(tmp_path / 'cp2')
    with caplog.at_level(logging.INFO, logger='traces'):
        example.traces([path], None, cp2, kind='sum', split=0.1, min_area=8)
    assert '0 of 5 ROIs split' in caplog.text
