"""Artefact frames without a GPU: the public names and the ABI, every ValueError in front of the library, flag_frames and
hold_index against the plain loops of tests/_frames_ref.py, the oracle against numpy, the reach table on the exact integer oracle
(three flash frames in a thousand blind the split rule and merge distinct cells; the filter gives both back), and
csrc/frame_math.h as a stand-alone program under the host sanitizers."""
import inspect
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _detrend_ref as dref
import _frames_ref as ref
import _merge_ref as mref
import _pair_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES = ('dc_frame_moments', 'dc_frame_quality', 'dc_frame_gather')


def test_public_names_and_abi():
    import deep_calcium_amd
    from deep_calcium_amd import _build, _gen_tape, _lib, footprints, frames, merge, roi_pairs, series
    for name in ('FrameQuality', 'FrameFilter', 'frame_quality_device', 'flag_frames', 'hold_index'):
        assert getattr(deep_calcium_amd, name) is getattr(frames, name) and name in deep_calcium_amd.__all__
    assert _lib.header_abi_version() >= 124 and 'frame_quality.hip' in _build.SOURCES
    assert '-ffp-contract=off' in _build.FILE_FLAGS['frame_quality.hip']
    protos = _lib.parse_header()
    tapeable = set(n for n, _ in _gen_tape.prototypes())
    for name in LAUNCHES:
        assert name in protos and name in tapeable, name
    assert [len(protos[n][1]) for n in LAUNCHES] == [12, 8, 8]
    assert open(_gen_tape.OUT).read() == _gen_tape.render()                 # the committed trampolines are current
    header = open(_lib.HEADER).read()
    assert 'Frame quality' in header and '#define DC_FRAME_MAX_PIXELS 268435456L' in header
    assert frames.MAX_PIXELS == ref.MAX_PIXELS == 2 ** 28 and frames.KINDS == ('moments', 'mean', 'corr')
    for f in ('frame_quality.hip', 'frame_math.h'):
        assert '#pragma clang fp contract(off)' in open(os.path.join(ROOT, 'deep_calcium_amd', 'csrc', f)).read()
    # keep= is None by default wherever frames are correlated, and absent where a trace needs every frame
    from deep_calcium_amd import dff, traces
    for fn in (series.summarize_series_device, footprints.roi_footprints_device, roi_pairs.roi_pair_corr_device, roi_pairs.split_rois_device,
               merge.merge_rois_device):
        assert inspect.signature(fn).parameters['keep'].default is None, fn.__name__
    for fn in (traces.extract_traces_device, dff.dff_traces_device):
        assert 'keep' not in inspect.signature(fn).parameters, fn.__name__
    assert list(inspect.signature(frames.FrameQuality.__init__).parameters)[1:] == ['shape', 'n_frames', 'dtype', 'template', 'rect', 'shifts',
                                                                                   'fine_shifts', 'bidi', 'device', 'chunk_frames']
    assert list(inspect.signature(frames.FrameFilter.__init__).parameters)[1:] == ['shape', 'n_frames', 'dtype', 'keep', 'shifts', 'fine_shifts',
                                                                                  'bidi', 'device', 'chunk_frames']


def test_module_imports_without_torch_or_the_library():
    code = ("import sys, deep_calcium_amd.frames as m; "
            "assert 'torch' not in sys.modules and 'deep_calcium_amd._lib' not in sys.modules; print(','.join(m.KINDS))")
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == 'moments,mean,corr', out.stderr[-500:]


# ---- every ValueError -----------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_the_library_is_touched(monkeypatch, tmp_path):
    from deep_calcium_amd import _lib, flag_frames, footprints, frames, hold_index, merge, roi_pairs, series

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'lib', boom)
    Q, F = frames.FrameQuality, frames.FrameFilter
    keep8 = np.ones(8, bool)
    for args, kw, what in ((((5, 7), 8, np.float32), {}, 'int16 or uint16'),
                           (((5,), 8, np.int16), {}, 'shape'),
                           (((5, 7), 0, np.int16), {}, 'n_frames'),
                           (((5, 7), 8, np.int16), {'chunk_frames': 0}, 'chunk_frames'),
                           (((5, 7), 8, np.int16), {'bidi': 7}, 'bidi'),
                           (((5, 7), 8, np.int16), {'shifts': np.zeros((7, 2), np.int32)}, 'shifts'),
                           (((5, 7), 8, np.int16), {'shifts': np.zeros((8, 2), np.int32), 'fine_shifts': np.zeros((8, 2), np.int32)}, 'not both')):
        with pytest.raises(ValueError, match=what):
            Q(*args, **kw)
        with pytest.raises(ValueError, match=what):
            F(*args, keep=keep8, **kw)
    # rect: outside the frame, empty, malformed
    for rect, what in ((((0, 6), (0, 7)), 'outside'), (((0, 5), (0, 8)), 'outside'), (((-1, 5), (0, 7)), 'outside'), (((0, 5), (-2, 7)), 'outside'),
                       (((2, 2), (0, 7)), 'empty'), (((0, 5), (4, 3)), 'empty'), (((0, 5),), 'rect must be'), ((0, 5, 0, 7), 'rect must be'),
                       (((0.0, 5.0), (0, 7)), 'integers'), (((0, True), (0, 7)), 'integers'), ('ab', 'rect must be')):
        with pytest.raises(ValueError, match=what):
            Q((5, 7), 8, np.int16, rect=rect)
    # n > 2^28: the whole frame, and a rectangle one column too wide
    with pytest.raises(ValueError, match=r'%d pixels: limited to 2\*\*28' % 2 ** 29):
        Q((2 ** 15, 2 ** 14), 8, np.int16)
    with pytest.raises(ValueError, match=r'%d pixels: limited to 2\*\*28' % (2 ** 28 + 2 ** 14)):
        Q((2 ** 15, 2 ** 15), 8, np.uint16, rect=((0, 2 ** 14), (5, 5 + 2 ** 14 + 1)))
    assert frames._check_rect(((0, 2 ** 14), (5, 5 + 2 ** 14)), (2 ** 15, 2 ** 15)) == (0, 2 ** 14, 5, 5 + 2 ** 14)        # 2^28 itself is served
    assert frames._check_rect(None, (5, 7)) == (0, 5, 0, 7) and frames._check_rect(((np.int64(1), 3), (2, np.int32(4))), (5, 7)) == (1, 3, 2, 4)
    # the template
    for bad in (np.zeros((5, 8), np.int16), np.zeros((5, 7), np.uint16), np.zeros((5, 7), np.float32), np.zeros((1, 5, 7), np.int16)):
        with pytest.raises(ValueError, match='template'):
            Q((5, 7), 8, np.int16, template=bad)
    # keep: the wrong length, nothing kept, not booleans
    for bad, what in ((np.ones(7, bool), 'keep has 7 entries, the recording has 8'), (np.ones(9, bool), 'keep has 9'), (np.zeros(8, bool), 'keeps no frame'),
                      (np.ones(8, np.int32), 'booleans'), (np.ones((8, 1), bool), 'booleans'), (None, 'booleans'), (np.ones(8, np.float64), 'booleans')):
        with pytest.raises(ValueError, match=what):
            F((5, 7), 8, np.int16, bad)
    with pytest.raises(ValueError, match='keeps no frame'):
        hold_index(np.zeros(4, bool))
    with pytest.raises(ValueError, match='booleans'):
        hold_index([1, 0, 1])
    # the one-call functions: a bad keep is refused before the file is opened, its length once the recording's is known
    rois = [np.array([[1, 1], [1, 2], [2, 1], [2, 2]]), np.array([[1, 3], [2, 3]])]
    calls = ((lambda **kw: series.summarize_series_device('/nonexistent/dataset.npz', kind='corr', **kw)),
             (lambda **kw: footprints.roi_footprints_device('/nonexistent/dataset.npz', rois, **kw)),
             (lambda **kw: roi_pairs.roi_pair_corr_device('/nonexistent/dataset.npz', rois, **kw)),
             (lambda **kw: roi_pairs.split_rois_device('/nonexistent/dataset.npz', rois, **kw)),
             (lambda **kw: merge.merge_rois_device('/nonexistent/dataset.npz', rois, **kw)))
    for call in calls:
        with pytest.raises(ValueError, match='keeps no frame'):
            call(keep=np.zeros(8, bool))
        with pytest.raises(ValueError, match='booleans'):
            call(keep=np.arange(8))
    path = str(tmp_path / 'recording.npz')
    np.savez(path, series_raw=np.zeros((8, 5, 7), np.int16))
    for fn, args in ((series.summarize_series_device, ()), (footprints.roi_footprints_device, (rois,)), (roi_pairs.roi_pair_corr_device, (rois,)),
                     (roi_pairs.split_rois_device, (rois,), ), (merge.merge_rois_device, (rois,))):
        kw = dict(min_area=1) if fn is roi_pairs.split_rois_device else {}
        with pytest.raises(ValueError, match='keep has 7 entries, the recording has 8'):
            fn(path, *args, keep=np.ones(7, bool), **kw)
    with pytest.raises(ValueError, match='bin_frames = 4, the recording has only 3'):            # b counts KEPT frames
        series.summarize_series_device(path, kind='corr', keep=np.array([1, 1, 1, 0, 0, 0, 0, 0], bool), bin_frames=4)
    # flag_frames
    for bad in (0, -1.0, float('nan'), float('inf'), True, None, '8'):
        with pytest.raises(ValueError, match='k must be'):
            flag_frames([1.0, 2.0, 3.0], k=bad)
    with pytest.raises(ValueError, match='mean must be'):
        flag_frames(np.zeros((3, 2)))
    with pytest.raises(ValueError, match='mean must be'):
        flag_frames([])
    with pytest.raises(ValueError, match='corr must have the shape'):
        flag_frames([1.0, 2.0, 3.0], [1.0, 2.0])
    with pytest.raises(ValueError, match='not finite'):
        flag_frames([1.0, float('nan'), 3.0])
    with pytest.raises(ValueError, match='kind'):
        frames._check_kind('std')


def test_inside_the_limits_the_arguments_reach_the_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from deep_calcium_amd import FrameFilter, FrameQuality
    from deep_calcium_amd._lib import DcunetError
    with pytest.raises(DcunetError, match='no CPU fallback'):
        FrameQuality((2 ** 15, 2 ** 15), 8, np.uint16, rect=((0, 2 ** 14), (5, 5 + 2 ** 14)))
    with pytest.raises(DcunetError, match='no CPU fallback'):
        FrameFilter((5, 7), 8, np.int16, np.array([0, 0, 0, 1, 0, 0, 0, 0], bool))


# ---- the rules on the host ----------------------------------------------------------------------------------------------------------
def test_flag_frames_on_hand_made_vectors_equals_the_plain_loops():
    from deep_calcium_amd import flag_frames
    # an outlier up, an outlier down, nothing else: med = 10, MAD = 1 -> s = 1.4826; 8 s = 11.86
    mean = [10.0, 11.0, 9.0, 10.0, 12.0, 8.0, 10.0, 22.0, -2.0, 21.8, 11.0, 9.0]
    keep = flag_frames(mean)
    assert keep.dtype == np.bool_ and keep.shape == (12,)
    assert keep.tolist() == ref.flag_frames(mean) == [True] * 7 + [False, False, True, True, True]            # 21.8 - 10 = 11.8 stays
    assert flag_frames(mean, k=11.0).tolist() == ref.flag_frames(mean, k=11.0) and flag_frames(mean, k=11.0).all()
    assert flag_frames(mean, k=0.5).tolist() == ref.flag_frames(mean, k=0.5)
    # corr: only a LOW value drops a frame
    corr = [0.90, 0.91, 0.89, 0.90, 0.92, 0.88, 0.90, 0.90, 0.90, 0.90, 0.99999, 0.5]
    both = flag_frames(mean, corr)
    assert both.tolist() == ref.flag_frames(mean, corr) == [True] * 7 + [False, False, True, True, False]
    # s == 0: every frame that differs from the median goes, however little
    flat = [5.0] * 6 + [5.0 + 2.0 ** -40, 4.0, 5.0]
    assert flag_frames(flat).tolist() == ref.flag_frames(flat) == [True] * 6 + [False, False, True]
    assert flag_frames([3.0]).tolist() == [True] and flag_frames([3.0, 3.0], [0.0, 0.0]).all()
    assert flag_frames(flat, [1.0] * 8 + [1.0 - 2.0 ** -30]).tolist() == [True] * 6 + [False, False, False]
    # ties at the median, an even count: the median is the mean of the two middle values
    tied = [1.0, 1.0, 2.0, 2.0, 1.0, 2.0, 40.0, 1.5]
    assert flag_frames(tied).tolist() == ref.flag_frames(tied) == [True] * 6 + [False, True]
    assert flag_frames([1.0, 3.0]).all()                                                                  # med 2, s = 1.4826: both within
    # float32 in (what the device returns), float64 arithmetic
    rs = np.random.RandomState(4)
    for trial in range(50):
        T = rs.randint(1, 60)
        m = (400 + 5 * rs.standard_normal(T)).astype(np.float32)
        c = (0.7 + 0.02 * rs.standard_normal(T)).astype(np.float32)
        if T > 4:
            m[rs.randint(T)] += 200
            c[rs.randint(T)] -= 0.5
        k = float(rs.choice([3.0, 8.0, 0.7]))
        assert flag_frames(m, c, k=k).tolist() == ref.flag_frames(m, c, k), trial
        assert flag_frames(m, k=k).tolist() == ref.flag_frames(m, None, k), trial


def test_hold_index_on_hand_made_vectors_equals_the_plain_loop():
    from deep_calcium_amd import hold_index
    for keep, want in (([1, 1, 1], [0, 1, 2]),
                       ([0, 0, 1, 1, 0, 1, 0, 0], [2, 2, 2, 3, 3, 5, 5, 5]),         # a leading and a trailing dropped run
                       ([1, 0, 0, 0], [0, 0, 0, 0]), ([0, 0, 0, 1], [3, 3, 3, 3]), ([1], [0]), ([0, 1, 0, 1, 0], [1, 1, 1, 3, 3])):
        got = hold_index(np.array(keep, bool))
        assert got.dtype == np.int64 and got.tolist() == want == ref.hold_index(keep), keep
    rs = np.random.RandomState(6)
    for trial in range(40):
        keep = rs.rand(rs.randint(1, 50)) < 0.6
        keep[rs.randint(len(keep))] = True
        h = hold_index(keep)
        assert h.tolist() == ref.hold_index(keep) and keep[h].all() and np.array_equal(h[keep], np.flatnonzero(keep))
    # the use: sums[:, hold_index(keep)] holds the last good sample
    sums = np.arange(16, dtype=np.int64).reshape(2, 8)
    keep = np.array([0, 1, 1, 0, 0, 1, 1, 0], bool)
    assert sums[:, hold_index(keep)].tolist() == [[1, 1, 2, 2, 2, 5, 6, 6], [9, 9, 10, 10, 10, 13, 14, 14]]


# ---- the oracle itself ----------------------------------------------------------------------------------------------------------------
def test_oracle_is_numpy_on_small_numbers():
    rs = np.random.RandomState(3)
    for dtype in (np.int16, np.uint16):
        info = np.iinfo(dtype)
        frames = rs.randint(info.min, info.max + 1, size=(6, 5, 9)).astype(dtype)
        tmpl = rs.randint(info.min, info.max + 1, size=(5, 9)).astype(dtype)
        for rect in (None, ((1, 4), (3, 8)), ((4, 5), (8, 9))):
            assert ref.moments(frames, tmpl, rect) == ref.moments_np(frames, tmpl, rect)
            assert ref.moments(frames, None, rect) == ref.moments_np(frames, None, rect) and all(m[2] == 0 for m in ref.moments(frames, None, rect))
            mom, mean, corr = ref.scores(frames, tmpl, rect)
            (y0, y1), (x0, x1) = ref.rect_of((5, 9), rect)
            x = frames[:, y0:y1, x0:x1].astype(np.float64).reshape(6, -1)
            t = tmpl[y0:y1, x0:x1].astype(np.float64).reshape(-1)
            assert mom.dtype == np.int64 and mom.shape == (6, 3) and np.array_equal(mom[:, 0], x.sum(1).astype(np.int64))
            assert np.allclose(mean, x.mean(1), rtol=1e-7, atol=0)
            if x.shape[1] > 1:
                assert np.allclose(corr, [np.corrcoef(r, t)[0, 1] for r in x], rtol=0, atol=1e-6)
            else:
                assert (corr == 0).all()                                                # n == 1: nothing varies
    g = np.arange(12, dtype=np.int16).reshape(3, 2, 2)
    assert ref.gather(g, [2, 0, 3, -1, 1]).tolist() == [g[2].tolist(), g[0].tolist(), [[0, 0], [0, 0]], [[0, 0], [0, 0]], g[1].tolist()]
    assert ref.gather(g, []).shape == (0, 2, 2)
    t = ref.template_of(np.array([[[1]], [[2]], [[2]], [[-4]]], np.int16))
    assert t.dtype == np.int16 and t.tolist() == [[0]] and ref.template_of(np.array([[[1]], [[2]]], np.int16)).tolist() == [[2]]        # half up


# ---- the reach of the rule, on the exact oracle ---------------------------------------------------------------------------------------
SEEDS = range(40)


def _corr64(N):
    """float64 quotients of the exact numerators standing in for the device: N_ij / sqrt(N_ii N_jj), 0 for a flat pixel."""
    N = N.astype(np.float64)
    d = np.diag(N).copy()
    ok = d > 0
    den = np.sqrt(np.where(ok, d, 1.0))
    C = N / den[:, None] / den[None, :]
    C[~ok] = 0
    C[:, ~ok] = 0
    return C


def _split(frames, region, left, right):
    """-> (the region was split, a pixel is on the wrong side or lost)."""
    from deep_calcium_amd import split_rois
    C = _corr64(dref.pooled_gram(frames[:, region[:, 0], region[:, 1]], frames.shape[0]))
    new, _, _ = split_rois([region], [C], frames.shape[1:], min_gap=0.1, min_area=8, iterations=16)
    if len(new) != 2:
        return False, False
    sets = [set(map(tuple, p.tolist())) for p in new]
    want = [set(map(tuple, left.tolist())), set(map(tuple, right.tolist()))]
    return True, sets != want


def _halves_merge(frames, left, right):
    f = frames.astype(np.int64)
    x, y = f[:, left[:, 0], left[:, 1]].sum(1).tolist(), f[:, right[:, 0], right[:, 1]].sum(1).tolist()
    return float(mref.corr64(mref.moments([x, y], [(0, 1)], None))[0]) >= 0.8


def test_reach_table_flash_frames_blind_the_rules_and_the_filter_gives_them_back():
    """_pair_ref.scene(kind, seed, 60, 30, T = 1024), seeds 0..39, 3 frames raised by 2000 grey levels (_frames_ref.plant).  The
    scores are the oracle's (exact moments over the whole 10 x 16 frame, the template the rounded mean of the first 200 frames of
    the recording WITH the flashes), the rule is flag_frames(mean, corr) at k = 8.  Measured here: all 480 planted frames flagged,
    82 of the 163 360 clean frames flagged with them (0.05 %); `two` split in 40 / 0 / 40 of 40 scenes (clean / flashes /
    filtered) with no pixel wrong, its halves merged at 0.8 in 0 / 40 / 0; the halves of `same` merged in 40 / 40 / 40; `same`,
    `gauss` and `static` split in 0 of 120 in every column."""
    from deep_calcium_amd import flag_frames
    planted = missed = clean = wrongly = 0
    split = dict((k, [0, 0, 0]) for k in pref.SCENES)
    wrong = dict((k, [0, 0, 0]) for k in pref.SCENES)
    merged = dict((k, [0, 0, 0]) for k in ('two', 'same'))
    for kind in pref.SCENES:
        for seed in SEEDS:
            frames, region, left, right, _ = pref.scene(kind, seed, 60.0, 30.0, T=1024)
            flashed, idx = ref.plant(frames, seed)
            _, mean, corr = ref.scores(flashed, ref.template_of(flashed), None, mom=ref.moments_np)
            keep = flag_frames(mean, corr)
            assert keep.tolist() == ref.flag_frames(mean, corr)
            planted += len(idx)
            missed += int(keep[idx].sum())
            clean += len(keep) - len(idx)
            wrongly += int((~keep).sum()) - int((~keep[idx]).sum())
            for col, f in enumerate((frames, flashed, flashed[keep])):
                s, w = _split(f, region, left, right)
                split[kind][col] += s
                wrong[kind][col] += w
                if kind in merged:
                    merged[kind][col] += _halves_merge(f, left, right)
    print('planted %d, missed %d; clean frames %d, wrongly flagged %d (%.3f %%)' % (planted, missed, clean, wrongly, 100.0 * wrongly / clean))
    print('%-44s %6s %8s %9s' % ('', 'clean', 'flashes', 'filtered'))
    print('%-44s %6d %8d %9d' % (('two: scenes split of 40',) + tuple(split['two'])))
    print('%-44s %6d %8d %9d' % (('two: split with a pixel wrong',) + tuple(wrong['two'])))
    print('%-44s %6d %8d %9d' % (('same / gauss / static: split of 120',) + tuple(sum(split[k][c] for k in ('same', 'gauss', 'static')) for c in range(3))))
    print('%-44s %6d %8d %9d' % (('two: halves merged at 0.8 of 40',) + tuple(merged['two'])))
    print('%-44s %6d %8d %9d' % (('same: halves merged at 0.8 of 40',) + tuple(merged['same'])))
    assert planted == 480 and missed == 0
    assert wrongly < 0.002 * clean                     # the rule does not "work" by dropping activity
    assert split['two'] == [40, 0, 40] and wrong['two'] == [0, 0, 0]
    assert merged['two'] == [0, 40, 0] and merged['same'] == [40, 40, 40]
    for kind in ('same', 'gauss', 'static'):
        assert split[kind] == [0, 0, 0], kind


# ---- the scalar arithmetic of the kernels --------------------------------------------------------------------------------------
def test_frame_math_under_the_host_sanitizers(tmp_path):
    """csrc/frame_math.h compiled into tests/native/frame_math_check.cpp with the address and undefined-behaviour sanitizers and
    run as a program of its own: the numerators against __int128 at the bounds (every pixel 65535 or -32768, n = 2^28) and on
    random moments, the exact cases of the correlation, the rectangle and the mean."""
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
    exe = str(tmp_path / 'frame_math_check')
    src = os.path.join(ROOT, 'tests', 'native', 'frame_math_check.cpp')
    r = subprocess.run([cxx] + flags + [src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'frame_math_check: ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_frames_of_one_call_are_limited(dclib):
    """DC_FRAMES_PER_CALL_MAX: tc = 2^30 + 1 is refused with (-3) and the limit's message before any launch, tc = 2^30 is not."""
    import _wideindex
    _wideindex.check_frame_limit(dclib, 'test_frames_api')
