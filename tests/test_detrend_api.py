"""Detrended (segment-pooled) correlations without a GPU: the public names and the ABI, the segment plan, argument validation in
front of and inside the library, the oracle of tests/_detrend_ref.py against its own definition and against today's numerators,
the reach of the split rule on bleached scenes (the table of the README), the conditions tests/test_detrend_gpu.py relies on, and
csrc/detrend_math.h as a stand-alone program under the host sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _detrend_ref as ref
import _pair_ref as pair_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES = ('dc_series_fold_segment', 'dc_series_finalize_pooled', 'dc_roi_pair_fold_segment', 'dc_roi_pair_corr_pooled',
            'dc_roi_pixel_fold_segment', 'dc_roi_pixel_corr_pooled')


def test_public_names_and_abi():
    import deep_calcium_amd
    from deep_calcium_amd import _build, _gen_tape, _lib, series
    assert deep_calcium_amd.detrend_plan is series.detrend_plan and 'detrend_plan' in deep_calcium_amd.__all__
    assert _lib.header_abi_version() >= 122
    protos = _lib.parse_header()
    tapeable = set(n for n, _ in _gen_tape.prototypes())
    for name in LAUNCHES:
        assert name in protos and name in tapeable, name
    assert [len(protos[n][1]) for n in LAUNCHES] == [13, 11, 13, 8, 15, 11]
    header = open(_lib.HEADER).read()
    assert 'Detrended correlations' in header and '#define DC_DETREND_MAX_FRAMES 4096' in header
    assert series.MAX_DETREND_FRAMES == ref.MAX_FRAMES == 4096 and series.MIN_DETREND_FRAMES == 2 and series.MAX_DETREND_VOLUME == 2 ** 46
    for f in ('series.hip', 'roi_pairs.hip', 'footprints.hip'):
        assert '-ffp-contract=off' in _build.FILE_FLAGS[f], f
        src = open(os.path.join(ROOT, 'deep_calcium_amd', 'csrc', f)).read()
        assert '#pragma clang fp contract(off)' in src and '#include "detrend_math.h"' in src, f
    math_h = open(os.path.join(ROOT, 'deep_calcium_amd', 'csrc', 'detrend_math.h')).read()
    assert '#pragma clang fp contract(off)' in math_h and '#include "pair_math.h"' in math_h
    # the keyword is where the issue puts it, and nowhere else
    import inspect
    from deep_calcium_amd import dff, footprints, roi_pairs, traces
    for fn in (series.SeriesSummarizer.__init__, roi_pairs.RoiPairCorr.__init__, footprints.RoiFootprints.__init__,
               series.summarize_series_device, footprints.roi_footprints_device, roi_pairs.roi_pair_corr_device, roi_pairs.split_rois_device):
        assert inspect.signature(fn).parameters['detrend_frames'].default is None, fn
    for fn in (traces.extract_traces_device, dff.dff_traces_device, traces.RoiTraceExtractor.__init__, series.TemporalBinner.__init__):
        assert 'detrend_frames' not in inspect.signature(fn).parameters, fn


# ---- the plan ----------------------------------------------------------------------------------------------------------------
def test_the_segment_plan():
    from deep_calcium_amd import detrend_plan
    assert detrend_plan(15, 8) == [(0, 15, 1)] and detrend_plan(5, 8) == [(0, 5, 1)] and detrend_plan(8, 8) == [(0, 8, 1)]      # T < 2 L
    assert detrend_plan(16, 8) == [(0, 8, 8), (8, 8, 8)]                                                                     # T = n L
    assert detrend_plan(32, 8) == [(0, 8, 8), (8, 8, 8), (16, 8, 8), (24, 8, 8)]
    assert detrend_plan(37, 8) == [(0, 8, 13), (8, 8, 13), (16, 8, 13), (24, 13, 8)]                                         # ragged
    assert detrend_plan(256, 100) == [(0, 100, 156), (100, 156, 100)]
    assert detrend_plan(1, 2) == [(0, 1, 1)]
    rs = np.random.RandomState(0)
    for T, L in [(int(t), int(l)) for t, l in zip(rs.randint(1, 40000, 300), rs.randint(2, 4097, 300))] + [(2 ** 31 - 1, 4096), (8191, 4096), (8192, 4096)]:
        got = detrend_plan(T, L)
        assert got == ref.plan(T, L)
        assert got[0][0] == 0 and all(a[0] + a[1] == b[0] for a, b in zip(got, got[1:])) and got[-1][0] + got[-1][1] == T
        M = got[0][1] * got[0][2]
        assert all(length * mult == M for _, length, mult in got) and M == ref.big_m(T, L)
        if len(got) > 1:
            assert all(length == L for _, length, _ in got[:-1]) and L <= got[-1][1] < 2 * L and M == L * got[-1][1]
        else:
            assert T < 2 * L and M == T
    for bad in ((0, 4), (4, 0)):
        with pytest.raises(ValueError):
            detrend_plan(*bad)


def test_a_chunk_is_cut_at_the_segment_boundaries():
    from deep_calcium_amd.series import _Segments
    seg = _Segments(37, 8)
    assert (seg.M, seg.n, seg.last) == (8 * 13, 4, 13)
    for chunk in (1, 5, 8, 37):
        t, seen, folded = 0, [], []
        while t < 37:
            tc = min(chunk, 37 - t)
            for k, m, within, ends in seg.cut(t, tc):
                assert m >= 1 and 0 <= k and k + m <= tc
                seen += list(range(t + k, t + k + m))
                s = min((t + k) // 8, 3)
                assert within == t + k - 8 * s                      # the frame's index within its segment: 0 initialises the state
                if ends is not None:
                    folded.append(ends)
                    assert t + k + m == ends[0] + ends[1]
            t += tc
        assert seen == list(range(37)) and folded == ref.plan(37, 8), chunk


# ---- validation ----------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    from deep_calcium_amd import _lib, footprints, roi_pairs, series

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'lib', boom)
    ok = [np.array([[1, 2], [3, 4]])]
    readers = ((lambda **kw: series.SeriesSummarizer((5, 7), 40, np.int16, **kw)),
               (lambda **kw: roi_pairs.RoiPairCorr((5, 7), 40, np.int16, ok, **kw)),
               (lambda **kw: footprints.RoiFootprints((5, 7), 40, np.int16, ok, **kw)),
               (lambda **kw: series.summarize_series_device('/nonexistent/dataset.npz', **kw)),
               (lambda **kw: footprints.roi_footprints_device('/nonexistent/dataset.npz', ok, **kw)),
               (lambda **kw: roi_pairs.roi_pair_corr_device('/nonexistent/dataset.npz', ok, **kw)),
               (lambda **kw: roi_pairs.split_rois_device('/nonexistent/dataset.npz', ok, **kw)))
    for make in readers:
        for bad, what in ((1, r'must be in \[2, 4096\]'), (4097, r'must be in \[2, 4096\]'), (0, r'must be in \[2, 4096\]'), (-8, r'must be in \[2, 4096\]'),
                          (2.0, 'must be an integer'), (True, 'must be an integer'), ('8', 'must be an integer'), ([8], 'must be an integer')):
            with pytest.raises(ValueError, match='detrend_frames ' + what):
                make(detrend_frames=bad)
    # M * H * W <= 2^46 against the declared n_frames: (2048, 4096) is 2^23 pixels, L = 4096 and T = 8192 give M = 2^24
    big = (2048, 4096)
    for make in ((lambda T, L: series.SeriesSummarizer(big, T, np.int16, detrend_frames=L)),
                 (lambda T, L: roi_pairs.RoiPairCorr(big, T, np.int16, ok, detrend_frames=L)),
                 (lambda T, L: footprints.RoiFootprints(big, T, np.int16, ok, detrend_frames=L))):
        for T, L in ((8192, 4096), (3 * 4096 + 5, 4096), (2 ** 22, 4095)):
            with pytest.raises(ValueError, match=r'M \* H \* W.*2\*\*46'):
                make(T, L)
    assert series._check_detrend_frames(2048, 8192, big) == 2048                          # M = 2^22: 2^45
    assert series._check_detrend_frames(np.int64(4096), 8192, (2048, 2048)) == 4096      # M * H * W = 2^46 exactly
    assert series._check_detrend_frames(4096, 8191, (2 ** 15, 2 ** 15)) == 4096            # one segment: M = T
    for kinds in (('mean16',), ('std', 'max16')):
        with pytest.raises(ValueError, match='mean16 / max16'):
            series.SeriesSummarizer((5, 7), 40, np.int16, kinds=kinds, detrend_frames=8)
    with pytest.raises(ValueError, match='mean16 / max16'):
        series.summarize_series_device('/nonexistent/dataset.npz', kind='mean16', detrend_frames=8)


def test_c_abi_argument_validation_returns_codes(dclib):
    """Refused before any launch (there is no GPU here): the pointers are never followed."""
    from deep_calcium_amd._lib import DcunetError
    L = dclib
    p = 4096                                  # any 16-byte aligned non-null value

    def SF(s=p, ss=p, xy=p, vm=p, n=8, mult=13, pv=p, pc=p, st=p, vt=p, H=5, W=7):
        return L.dc_series_fold_segment(s, ss, xy, vm, n, mult, pv, pc, st, vt, H, W, None)

    def SZ(pv=p, pc=p, st=p, mean=p, sd=p, corr=p, H=5, W=7, M=104, T=37):
        return L.dc_series_finalize_pooled(pv, pc, st, mean, sd, corr, H, W, M, T, None)

    def PF(a=p, g=p, off=p, goff=p, tiles=p, ntiles=0, R=1, P=4, G=16, n=8, mult=13, pooled=p):
        return L.dc_roi_pair_fold_segment(a, g, off, goff, tiles, ntiles, R, P, G, n, mult, pooled, None)

    def PC(pooled=p, off=p, goff=p, R=0, P=4, G=16, corr=p):
        return L.dc_roi_pair_corr_pooled(pooled, off, goff, R, P, G, corr, None)

    def XF(mom=p, N=4, off=p, roi=p, S=1, R=0, rmom=p, n=8, mult=13, xx=p, xs=p, ss=p, H=5, W=7):
        return L.dc_roi_pixel_fold_segment(mom, N, off, roi, S, R, rmom, n, mult, xx, xs, ss, H, W, None)

    def XC(xx=p, xs=p, ss=p, N=0, off=p, roi=p, S=1, R=1, inside=p, corr=p):
        return L.dc_roi_pixel_corr_pooled(xx, xs, ss, N, off, roi, S, R, inside, corr, None)
    nulls = ((SF, ('s', 'ss', 'vm', 'pv', 'st', 'vt')), (SZ, ('pv',)), (PF, ('a', 'g', 'off', 'goff', 'tiles', 'pooled')),
             (PC, ('pooled', 'off', 'goff', 'corr')), (XF, ('mom', 'off', 'rmom', 'xx', 'xs', 'ss')), (XC, ('xx', 'xs', 'ss', 'off', 'inside', 'corr')))
    for fn, names in nulls:
        for name in names:
            with pytest.raises(DcunetError, match=r'\(-1\).*null'):
                fn(**{name: None})
    with pytest.raises(DcunetError, match=r'\(-1\).*come as a pair'):
        SF(xy=None)
    with pytest.raises(DcunetError, match=r'\(-1\).*corr needs'):
        SZ(pc=None)
    with pytest.raises(DcunetError, match=r'\(-1\).*mean needs'):
        SZ(st=None)
    # a pooled word is a 16-byte element: an 8-byte aligned pointer is refused
    for fn, names in ((SF, ('pv', 'pc')), (SZ, ('pv', 'pc')), (PF, ('pooled',)), (PC, ('pooled',)), (XF, ('xx', 'xs', 'ss')), (XC, ('xx', 'xs', 'ss'))):
        for name in names:
            with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
                fn(**{name: p + 8})
    for fn, names in ((SF, ('s', 'ss', 'xy', 'st')), (PF, ('a', 'g', 'goff')), (XF, ('mom', 'rmom'))):
        for name in names:
            with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
                fn(**{name: p + 4})
    for fn in (SF, PF, XF):
        for kw in (dict(n=0), dict(n=-3), dict(mult=0), dict(mult=-1)):
            with pytest.raises(DcunetError, match=r'\(-1\).*a segment of'):
                fn(**kw)
        for kw in (dict(n=8192, mult=2), dict(n=2, mult=8192), dict(n=2 ** 31, mult=1)):
            with pytest.raises(DcunetError, match=r'\(-3\).*limited to 8191 frames'):
                fn(**kw)
    for fn in (SF, XF):
        with pytest.raises(DcunetError, match=r'\(-1\).*out of range'):
            fn(H=2 ** 15, W=2 ** 15 + 1)
        with pytest.raises(DcunetError, match=r'\(-3\).*M \* H \* W is limited to 2\^46'):
            fn(n=4096, mult=4096, H=2048, W=4096)
    with pytest.raises(DcunetError, match=r'\(-3\).*M \* H \* W is limited to 2\^46'):
        SZ(M=2 ** 24, T=8192, H=2048, W=4096)
    for kw in (dict(M=0), dict(T=0), dict(M=-1)):
        with pytest.raises(DcunetError, match=r'\(-1\).*M = '):
            SZ(**kw)
    with pytest.raises(DcunetError, match=r'\(-3\).*each is limited to'):
        SZ(T=2 ** 31)
    for fn in (PF, PC):
        for kw in (dict(R=-1), dict(P=-1), dict(G=-1)):
            with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
                fn(**kw)
        with pytest.raises(DcunetError, match=r'\(-3\).*2\^27 = 134217728'):
            fn(P=2 ** 18, G=2 ** 27 + 1)
        with pytest.raises(DcunetError, match=r'\(-3\).*more than 1024 pixels'):
            fn(P=4, G=4097)
    with pytest.raises(DcunetError, match=r'\(-3\).*137 tiles for 1 ROIs'):
        PF(ntiles=137)
    with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
        PF(ntiles=-1)
    for fn in (XF, XC):
        for kw in (dict(N=-1), dict(S=-1), dict(R=-1)):
            with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
                fn(**kw)
        with pytest.raises(DcunetError, match=r'\(-1\).*without row_roi'):
            fn(roi=None, S=2, R=1)
    # empty work: nothing launched
    assert PF() == 0 and PF(ntiles=1, P=0, G=0) == 0 and PC() == 0 and XF() == 0 and XC() == 0 and XC(N=4, S=0, R=0, roi=None) == 0


# ---- the oracle itself -----------------------------------------------------------------------------------------------------------
def _small(dtype=np.int16, T=37, H=4, W=5, seed=3):
    rs = np.random.RandomState(seed)
    info = np.iinfo(dtype)
    f = rs.randint(info.min, info.max + 1, size=(T, H, W)).astype(dtype)
    f[:, 0, 0] = np.where(np.arange(T) % 2, info.min, info.max)               # alternating extremes
    f[:, 0, 1] = info.max                                                     # constant
    f[:, 0, 2] = np.repeat([info.min, 5, info.max, -3 if info.min else 3, 0], 8)[:T]      # constant within every segment of 8 but the last
    return f


@pytest.mark.parametrize('dtype', [np.int16, np.uint16])
def test_the_vectorised_oracle_is_its_definition(dtype):
    f = _small(dtype)
    T, H, W = f.shape
    flat = f.reshape(T, -1)
    for L in (8, 5, 19, 40):
        var, cov = ref.series_numerators(f, L)
        gram = ref.pooled_gram(flat, L)
        for p in range(H * W):
            y, x = divmod(p, W)
            assert var[y, x] == gram[p][p] == ref.pooled_pair(flat[:, p], flat[:, p], L)
            for j, (dy, dx) in enumerate(ref.SLOTS):
                qy, qx = y + dy, x + dx
                want = ref.pooled_pair(flat[:, p], flat[:, qy * W + qx], L) if 0 <= qy < H and 0 <= qx < W else 0
                assert cov[j, y, x] == want and type(cov[j, y, x]) is int, (L, p, j)
        assert all(gram[i][j] == gram[j][i] for i in range(H * W) for j in range(H * W))
        own, support = [6, 7, 11, 12], [0, 1, 2, 5, 6, 7, 8, 10, 11, 12, 13, 16, 17, 18]
        cxx, cxs, css = ref.footprint_numerators(f, own, support, L)
        S = flat[:, own].astype(np.int64).sum(1)
        assert css == ref.pooled_pair(S, S, L)
        for e, p in enumerate(support):
            assert cxx[e] == gram[p][p] and cxs[e] == ref.pooled_pair(flat[:, p], S, L) == sum(gram[p][q] for q in own), (L, e)


@pytest.mark.parametrize('dtype', [np.int16, np.uint16])
def test_one_segment_gives_todays_numerators(dtype):
    """n == 1 (L > T / 2): N(x, y) = T g - a a', the integers dc_roi_pair_corr and dc_series_finalize form today."""
    f = _small(dtype)
    T = f.shape[0]
    flat = list(range(f.shape[1] * f.shape[2]))
    a, g = pair_ref.moments(f, flat)
    for L in (19, 37, 38, 4096):
        assert ref.plan(T, L) == [(0, T, 1)] and ref.big_m(T, L) == T
        N = ref.pooled_gram(f.reshape(T, -1), L)
        for i in flat:
            for j in flat:
                assert (N[i][i], N[i][j], N[j][j]) == pair_ref.numerators(T, a, g, i, j)
        assert np.array_equal(ref.pair_corr(N).view(np.int32), pair_ref.matrix(T, a, g).view(np.int32))
    assert ref.pooled_gram(f.reshape(T, -1), 18)[0][0] != pair_ref.numerators(T, a, g, 0, 0)[0]      # two segments: another integer


@pytest.mark.parametrize('dtype', [np.int16, np.uint16])
def test_symmetry_diagonal_and_flat_pixels(dtype):
    f = _small(dtype)
    T, H, W = f.shape
    N = ref.pooled_gram(f.reshape(T, -1), 8)
    C = ref.pair_corr(N)
    assert np.array_equal(C.view(np.int32), C.T.view(np.int32)) and (np.abs(C) <= 1).all()
    # pixel 1 is constant; pixel 2 is constant within the segments of 8 frames but varies within the last one (13 frames)
    assert N[1][1] == 0 and N[2][2] > 0
    varies = np.array([N[i][i] > 0 for i in range(H * W)])
    assert np.array_equal(np.diag(C), varies.astype(np.float32))
    assert not C[1].any() and not C[:, 1].any()
    g = f.copy()
    g[:, 0, 2] = np.repeat(np.array([7, 5, 9, 3], g.dtype), [8, 8, 8, 13])          # constant within EVERY segment, though not in time
    N = ref.pooled_gram(g.reshape(T, -1), 8)
    C = ref.pair_corr(N)
    assert N[2][2] == 0 and not C[2].any() and not C[:, 2].any() and all(N[2][j] == 0 for j in range(H * W))
    assert ref.pooled_gram(g.reshape(T, -1), 40)[2][2] > 0                             # the whole recording sees it vary
    # the series image of the same recording: the flat pixel counts 0 towards its neighbours' means, and is 0 itself
    var, cov = ref.series_numerators(g, 8)
    img = ref.series_corr(var, cov)
    assert img[0, 1] == 0 and img[0, 2] == 0 and np.isfinite(img).all() and (np.abs(img) <= 1).all()
    sd = ref.series_std(var, 8 * 13, T)
    assert sd[0, 1] == 0 and sd[0, 2] == 0 and sd[0, 0] > 0


def test_detrending_removes_a_step_between_segments_exactly():
    """A level that changes only at segment boundaries is invisible: the pooled numerators of x and of x + step are one integer."""
    rs = np.random.RandomState(9)
    T, L = 37, 8
    X = rs.randint(-300, 300, size=(T, 6))
    step = np.repeat([1000, -2000, 500, 12000], [8, 8, 8, 13])[:, None] * np.array([1, 2, 0, 1, 3, 1])[None, :]
    assert np.array_equal(ref.pooled_gram(X, L), ref.pooled_gram(X + step, L))
    assert not np.array_equal(ref.pooled_gram(X, T), ref.pooled_gram(X + step, T))


# ---- the reach of the split rule under bleaching ----------------------------------------------------------------------------------
def _corr64(N):
    """float64 pooled covariances standing in for the device: N_ij / sqrt(N_ii N_jj), 0 for a flat pixel."""
    N = N.astype(np.float64)
    d = np.diag(N).copy()
    ok = d > 0
    den = np.sqrt(np.where(ok, d, 1.0))
    C = N / den[:, None] / den[None, :]
    C[~ok] = 0
    C[:, ~ok] = 0
    return C


def _wrong(new, left, right):
    sets = [set(map(tuple, p.tolist())) for p in new]
    want = [set(map(tuple, left.tolist())), set(map(tuple, right.tolist()))]
    return len(sets[0] - want[0]) + len(sets[1] - want[1]), len((want[0] | want[1]) - (sets[0] | sets[1]))


def _reach(kind, amplitude, sigma, beta, L, T=1024):
    """-> (scenes split of 40, scenes split with a pixel misassigned or dropped)."""
    from deep_calcium_amd import split_rois
    split = bad = 0
    for seed in range(40):
        frames, region, left, right, _ = pair_ref.scene(kind, seed, amplitude, sigma, T=T)
        if beta is not None:
            frames = ref.bleach(frames, beta)
        C = _corr64(ref.pooled_gram(frames[:, region[:, 0], region[:, 1]], T if L is None else L))
        new, _, _ = split_rois([region], [C], frames.shape[1:], min_gap=0.1, min_area=8, iterations=16)
        if len(new) == 2:
            split += 1
            bad += _wrong(new, left, right) != (0, 0)
    return split, bad


def test_the_reach_of_the_split_rule_on_bleached_scenes():
    """The table of the README, regenerated from the oracle's numerators: the scene of _pair_ref.scene at T = 1024, 40 seeds,
    bleached to the fraction beta of its start, split with the whole-recording correlation (L = None) and within segments of
    128 frames.  Measured here: two cells at 60 / 30 -- 40/0 and 40/0 without decay, 0/0 and 40/0 with decay to 0.5; 0 of the 120
    controls split in either mode, with or without decay."""
    table = {}
    for beta in (None, 0.5):
        for L in (None, 128):
            table[beta, L] = _reach('two', 60.0, 30.0, beta, L)
    controls = {}
    for beta in (None, 0.5):
        for L in (None, 128):
            controls[beta, L] = sum(_reach(kind, 60.0, 30.0, beta, L)[0] for kind in ('same', 'gauss', 'static'))
    print('amplitude / sigma   decay to   whole recording   L = 128      (scenes split of 40 / with a pixel wrong)')
    for beta in (None, 0.5):
        print('60 / 30             %-8s   %2d/%d              %2d/%d' % ((beta or 'none',) + table[beta, None] + table[beta, 128]))
    for beta in (None, 0.5):
        print('controls (120)      %-8s   %2d                %2d' % (beta or 'none', controls[beta, None], controls[beta, 128]))
    assert table[0.5, None][0] <= 2                                   # bleached and undetrended: the rule is blind
    assert table[0.5, 128][0] >= 38 and table[0.5, 128][1] == 0       # bleached at L = 128: given back, no pixel wrong
    assert table[None, 128] == (40, 0) and table[None, None] == (40, 0)      # the undetrended scene loses nothing at L = 128
    assert all(v == 0 for v in controls.values()), controls


def test_the_bleached_gpu_scene_meets_its_conditions_on_the_reference():
    """What the end-to-end test of tests/test_detrend_gpu.py relies on, on the float64 oracle: _pair_ref.gpu_scene() bleached to
    0.5.  With the whole-recording correlation the two-cell region is NOT split and its gap stays below 0.08 (min_gap is 0.1);
    within segments of 64 frames it is split into the planted halves with a gap of at least 0.15; the controls' gaps stay below
    0.05 or undefined in both modes, and the strip is too small to be looked at."""
    from deep_calcium_amd import split_rois
    frames, rois, left, right = pair_ref.gpu_scene()
    frames = ref.bleach(frames, 0.5)
    assert frames.dtype == np.int16 and frames.shape == (256, 10, 64)
    assert 0.49 < frames[-8:].mean() / frames[:8].mean() < 0.53
    for L, splits in ((None, False), (64, True)):
        C = [_corr64(ref.pooled_gram(frames[:, r[:, 0], r[:, 1]], 256 if L is None else L)) for r in rois]
        for fn in (split_rois, pair_ref.split):
            new, origin, gaps = fn(rois, C, frames.shape[1:], min_gap=0.1, min_area=8, iterations=16)
            assert origin == ([0, 1, 1, 2, 3, 4] if splits else [0, 1, 2, 3, 4]), (L, origin)
            if splits:
                assert np.array_equal(new[1], left) and np.array_equal(new[2], right) and gaps[1] >= 0.15, gaps
            else:
                assert gaps[1] < 0.08, gaps
            assert np.isnan(gaps[2]) and all(not g >= 0.05 for g in gaps[[0, 3, 4]]), gaps


# ---- the scalar arithmetic of the kernels --------------------------------------------------------------------------------------
def test_detrend_math_under_the_host_sanitizers(tmp_path):
    """csrc/detrend_math.h compiled into tests/native/detrend_math_check.cpp with the address and undefined-behaviour sanitizers
    and run as a program of its own: the fold arithmetic against __int128 at the magnitude limits (|x| = 65535, L = 4096,
    L_last = 8191, the largest T and area the volume rules allow), one segment against today's numerators, the footprint rule on
    pooled numerators, and the acceptance of segments."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    # sanitizer runtimes linked statically (clang's default; gcc needs the flags): the program is then indifferent to whatever
    # the environment preloads, and the environment is passed through untouched
    flags = ['-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    probe = str(tmp_path / 'probe.cpp')
    with open(probe, 'w') as fp:
        fp.write('int main() { return 0; }\n')
    for extra in (['-static-libasan', '-static-libubsan'], []):
        r = subprocess.run([cxx] + flags + extra + [probe, '-o', str(tmp_path / 'probe')], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            flags += extra
            break
    else:
        pytest.skip('the host compiler cannot link the sanitizer runtimes: %s' % r.stderr[-300:])
    exe = str(tmp_path / 'detrend_math_check')
    src = os.path.join(ROOT, 'tests', 'native', 'detrend_math_check.cpp')
    r = subprocess.run([cxx] + flags + [src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'detrend_math_check: ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
