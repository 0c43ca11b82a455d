"""Bidirectional scan-phase correction without a GPU: argument validation in front of and inside the library, the host pick and its
ties, valid_rectangle(bidi=) against a brute-force mask, the header, the trampolines and the README's file list, and the reach
of the numpy oracle on the planted-offset recordings tests/test_bidi_gpu.py reuses."""
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import _bidi_ref as bref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _boom(*a, **k):
    raise AssertionError('the library was touched')


# ---- static checks ---------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_new_entry_points():
    from deep_calcium_amd import _build, _gen_tape, _lib, motion
    import deep_calcium_amd
    protos = _lib.parse_header()
    tapeable = dict(_gen_tape.prototypes())
    want = {'dc_bidi_scores': ['frames', 'is_unsigned', 'tc', 'H', 'W', 'P', 'scores', 'stream'],
            'dc_bidi_apply': ['frames', 'tc', 'p', 'H', 'W', 'fill', 'out', 'stream']}
    for name, args in want.items():
        assert name in protos and name in tapeable, name
        assert protos[name][2] == args and len(tapeable[name]) == len(args)
    assert open(_gen_tape.OUT).read() == _gen_tape.render()                 # the committed trampolines are current
    header = open(_lib.HEADER).read()
    assert 'DC_BIDI_MAX_OFFSET 16' in header and motion.MAX_BIDI == 16
    assert header.index('---- wide search') < header.index('---- bidirectional scan-phase correction') < header.index('---- UNet1D spike inference')
    assert _lib.header_abi_version() >= 120 and 'motion.hip' in _build.SOURCES
    # the new keyword is the last one everywhere, and 0 by default
    from deep_calcium_amd import dff, footprints, roi_pairs, series, traces
    for fn in (motion.MotionCorrector.__init__, motion.make_template, motion.estimate_shifts_device, motion.valid_rectangle,
               series.SeriesSummarizer.__init__, series.summarize_series_device, traces.RoiTraceExtractor.__init__,
               traces.extract_traces_device, footprints.RoiFootprints.__init__, footprints.roi_footprints_device,
               roi_pairs.RoiPairCorr.__init__, roi_pairs.roi_pair_corr_device, roi_pairs.split_rois_device, dff.dff_traces_device):
        params = list(inspect.signature(fn).parameters.values())
        assert params[-1].name == 'bidi' and params[-1].default == 0, fn
    assert list(inspect.signature(motion.BidiEstimator.__init__).parameters)[1:] == ['shape', 'dtype', 'max_offset', 'device', 'chunk_frames']
    assert list(inspect.signature(motion.estimate_bidi_device).parameters) == ['dspath', 'max_offset', 'frames', 'source', 'device']
    assert inspect.signature(motion.estimate_bidi_device).parameters['frames'].default == 200
    for name in ('BidiEstimator', 'pick_bidi', 'estimate_bidi_device'):
        assert getattr(deep_calcium_amd, name) is getattr(motion, name)
    # the documents: the subsection sits in front of the piecewise-rigid one and states the scope; the file list names the new files
    readme = open(os.path.join(ROOT, 'README.md')).read()
    assert readme.index('### Motion correction on the device') < readme.index('Bidirectional scan-phase correction') < readme.index('Piecewise-rigid')
    for text in (readme, motion.__doc__):
        assert 'A sub-pixel or per-frame offset is not built' in ' '.join(text.split()) or 'a sub-pixel or per-frame offset is not built' in ' '.join(text.split())
    for name in ('tests/_bidi_ref.py', 'tests/test_bidi_api.py', 'tests/test_bidi_gpu.py', 'scripts/bidi_speed.py'):
        assert name in readme and os.path.exists(os.path.join(ROOT, name)), name
    assert '4f' in open(os.path.join(ROOT, 'DESIGN.md')).read()


def test_motion_module_still_imports_without_torch_or_the_library():
    code = ("import sys, deep_calcium_amd.motion as m; "
            "assert 'torch' not in sys.modules and 'deep_calcium_amd._lib' not in sys.modules; print(m.MAX_BIDI, m.pick_bidi([3, 1, 2]))")
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == '16 0', out.stderr[-500:]


# ---- argument checks -------------------------------------------------------------------------------------------------------------------
def test_bidi_keyword_is_checked_before_the_library_is_touched(monkeypatch):
    from deep_calcium_amd import _lib, dff, footprints, motion, roi_pairs, series, traces
    monkeypatch.setattr(_lib, 'lib', _boom)
    H, W = 20, 24
    t = np.zeros((H, W), np.int16)
    rois = [np.array([[1, 1], [1, 2], [2, 1], [2, 2]])]
    makers = [lambda b: motion.MotionCorrector((H, W), 4, np.int16, t, bidi=b),
              lambda b: motion.make_template(np.zeros((3, H, W), np.int16), bidi=b),
              lambda b: motion.valid_rectangle(np.zeros((3, 2), np.int32), (H, W), bidi=b),
              lambda b: series.SeriesSummarizer((H, W), 4, np.int16, bidi=b),
              lambda b: traces.RoiTraceExtractor((H, W), 4, np.int16, rois, bidi=b),
              lambda b: footprints.RoiFootprints((H, W), 4, np.int16, rois, bidi=b),
              lambda b: roi_pairs.RoiPairCorr((H, W), 4, np.int16, rois, bidi=b)]
    for make in makers:
        for bad in (1.0, True, '2', None, (1,), np.float32(2)):
            with pytest.raises(ValueError, match='bidi must be an integer'):
                make(bad)
        for bad in (W, -W, W + 7, 2 ** 31):
            with pytest.raises(ValueError, match='bidi'):
                make(bad)
    # the one-call functions check the type before they open the file
    for fn in (lambda b: motion.estimate_shifts_device('/nonexistent/dataset.npz', bidi=b),
               lambda b: series.summarize_series_device('/nonexistent/dataset.npz', bidi=b),
               lambda b: traces.extract_traces_device('/nonexistent/dataset.npz', rois, bidi=b)):
        for bad in (1.5, False, 2 ** 31):
            with pytest.raises(ValueError, match='bidi'):
                fn(bad)
    # legal values reach the library
    for b in (0, 3, -3, np.int64(W - 1), -(W - 1)):
        with pytest.raises(AssertionError, match='the library was touched'):
            motion.MotionCorrector((H, W), 4, np.int16, t, bidi=b)
    assert motion.valid_rectangle(np.zeros((3, 2), np.int32), (H, W), bidi=np.int32(2)) == ((0, H), (0, W - 2))
    # the search radius
    E = motion.BidiEstimator
    for bad in (17, -1, 100):
        with pytest.raises(ValueError, match=r'max_offset must be in \[0, 16\], not %d' % bad):
            E((H, 64), np.int16, max_offset=bad)
        with pytest.raises(ValueError, match=r'max_offset must be in \[0, 16\]'):
            motion.estimate_bidi_device('/nonexistent/dataset.npz', max_offset=bad)
    for bad in (8.0, True, '8', None):
        with pytest.raises(ValueError, match='max_offset must be an integer'):
            E((H, 64), np.int16, max_offset=bad)
    for Wb, P in ((16, 8), (2, 1), (32, 16), (15, 8)):
        with pytest.raises(ValueError, match=r'max_offset = %d leaves no interior column in a %d x %d frame: W > 2 \* max_offset' % (P, H, Wb)):
            E((H, Wb), np.int16, max_offset=P)
    for Hb in (1, 2):
        with pytest.raises(ValueError, match=r'a %d x 64 frame has no odd line between two even ones: H >= 3' % Hb):
            E((Hb, 64), np.int16)
    with pytest.raises(ValueError, match='int16 or uint16'):
        E((H, 64), np.float32)
    with pytest.raises(ValueError, match='chunk_frames'):
        E((H, 64), np.int16, chunk_frames=0)
    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match='frames must be None or an integer >= 1'):
            motion.estimate_bidi_device('/nonexistent/dataset.npz', frames=bad)
    for kw in ({}, {'max_offset': 0}, {'max_offset': 16}, {'max_offset': np.int64(3)}):
        with pytest.raises(AssertionError, match='the library was touched'):
            E((3, 33), np.uint16, **kw)


def test_c_abi_argument_validation_returns_codes(dclib):
    """Refused before any launch (there is no GPU here): the pointers are never followed."""
    from deep_calcium_amd._lib import DcunetError
    p = 4096

    def sc_args(frames=p, uns=0, tc=1, H=9, W=40, P=4, scores=p):
        return (frames, uns, tc, H, W, P, scores, None)
    scores, apply = dclib.dc_bidi_scores, dclib.dc_bidi_apply
    for kw in ({'frames': None}, {'scores': None}):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            scores(*sc_args(**kw))
    for kw in ({'tc': -1}, {'P': -1}, {'H': 0}, {'W': -2}):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative or zero'):
            scores(*sc_args(**kw))
    for kw in ({'H': 2}, {'H': 1}, {'W': 8}, {'W': 32, 'P': 16}, {'W': 1, 'P': 1}):
        with pytest.raises(DcunetError, match=r'\(-1\).*H >= 3 and W > 2P'):
            scores(*sc_args(**kw))
    with pytest.raises(DcunetError, match=r'\(-3\).*limited to 16'):
        scores(*sc_args(P=17, W=100))
    with pytest.raises(DcunetError, match=r'\(-3\).*2\^28'):
        scores(*sc_args(H=2 ** 14, W=2 ** 14 + 1))
    for kw in ({'frames': p + 1}, {'scores': p + 4}):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            scores(*sc_args(**kw))
    assert scores(*sc_args(tc=0)) == 0 and scores(*sc_args(tc=0, P=0, H=3, W=1, uns=1)) == 0 and scores(*sc_args(tc=0, P=16, W=33)) == 0
    assert scores(*sc_args(tc=0, H=2 ** 14, W=2 ** 14)) == 0               # 2^28 itself is legal

    def ap_args(frames=p, tc=1, off=1, H=6, W=10, fill=0, out=16 * p):
        return (frames, tc, off, H, W, fill, out, None)
    for kw in ({'frames': None}, {'out': None}):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            apply(*ap_args(**kw))
    for kw in ({'tc': -1}, {'H': 0}, {'W': 0}):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative or zero'):
            apply(*ap_args(**kw))
    with pytest.raises(DcunetError, match=r'\(-3\).*2\^30'):
        apply(*ap_args(H=2 ** 15, W=2 ** 15 + 1, out=2 ** 40))
    for fill in (-32769, 65536):
        with pytest.raises(DcunetError, match=r'\(-1\).*not a 16-bit value'):
            apply(*ap_args(fill=fill))
    for kw in ({'frames': p + 1}, {'out': 16 * p + 1}):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            apply(*ap_args(**kw))
    for kw in ({'out': p}, {'out': p + 2 * 60 - 2}, {'frames': 16 * p, 'out': 16 * p - 2 * 60 + 2}, {'tc': 2, 'out': p + 2 * 60}):
        with pytest.raises(DcunetError, match=r'\(-1\).*out overlaps frames'):
            apply(*ap_args(**kw))
    for off in (0, 5, -2 ** 31, 2 ** 31 - 1):                               # any int32 offset is legal
        assert apply(*ap_args(tc=0, off=off)) == 0


# ---- the pick ------------------------------------------------------------------------------------------------------------------------
def test_the_pick_and_its_ties():
    from deep_calcium_amd.motion import pick_bidi
    assert pick_bidi([7] * 9) == 0 and pick_bidi([7]) == 0                  # all equal: 0
    t = [9] * 9
    t[4 - 2] = t[4 + 2] = 1
    assert pick_bidi(t) == -2                                               # p = +-2 equal: the negative one
    t[4 + 1] = 1
    assert pick_bidi(t) == 1                                                # the smaller |p| first
    t[4] = 1
    assert pick_bidi(t) == 0                                                # 0 wins every tie it is part of
    t[4 - 3] = 0
    assert pick_bidi(t) == -3                                               # the total comes first
    big = [2 ** 70 + 5, 2 ** 70 + 1, 2 ** 70 + 3, 2 ** 70 + 1, 2 ** 70 + 2]   # beyond 2^63; float64 could not tell them apart
    assert pick_bidi(big) == -1 and float(big[1]) == float(big[0])
    assert pick_bidi(np.array([5, 3, 4], np.int64)) == 0 and pick_bidi((np.int64(2), 1, 1)) == 0
    for bad in ([], [1, 2], [1, 2, 3, 4]):
        with pytest.raises(ValueError, match='2P\\+1'):
            pick_bidi(bad)
    rs = np.random.RandomState(0)
    for _ in range(200):
        P = int(rs.randint(0, 17))
        tot = [int(v) for v in rs.randint(0, 4, size=2 * P + 1)]
        assert pick_bidi(tot) == bref.pick(tot) == sorted(range(-P, P + 1), key=lambda p: (tot[p + P], p * p, p))[0]
    # the totals are exact sums: 2^61-sized scores of many frames do not wrap
    sc = np.full((9, 3), 2 ** 61 - 1, np.int64)
    assert bref.totals(sc) == [9 * (2 ** 61 - 1)] * 3 and bref.totals(sc)[0] > 2 ** 63


# ---- valid_rectangle(bidi=) -------------------------------------------------------------------------------------------------------------
def _brute(shifts, shape, p, fine):
    """The largest rectangle of output pixels that read only in-frame sources, from a mask: the output (y, x) of a frame at the
    shift (sy, sx) reads the moved lines at the used taps; a moved odd line at column c reads the frame at c + p, and with a y
    shift either parity of line may land on any output row."""
    H, W = shape
    ok = np.ones((H, W), bool)
    yy, xx = np.mgrid[0:H, 0:W]
    rows = [(0, 0)] if shifts is None else [tuple(int(v) for v in r) for r in np.asarray(shifts).reshape(-1, 2)]
    for sy, sx in rows:
        if fine and shifts is not None:
            ys, xs = {sy // 16, -((-sy) // 16)}, {sx // 16, -((-sx) // 16)}
        else:
            ys, xs = {sy}, {sx}
        for dy in ys:
            ok &= (yy + dy >= 0) & (yy + dy < H)
        for dx in xs:
            for q in (0, p):
                ok &= (xx + dx + q >= 0) & (xx + dx + q < W)
    rr, c = np.flatnonzero(ok.any(axis=1)), np.flatnonzero(ok.any(axis=0))
    if not len(rr) or not len(c):
        return None
    assert ok[rr[0]:rr[-1] + 1, c[0]:c[-1] + 1].all() and ok.sum() == len(rr) * len(c)      # the mask IS a rectangle
    return (int(rr[0]), int(rr[-1]) + 1), (int(c[0]), int(c[-1]) + 1)


def test_valid_rectangle_with_bidi_against_a_brute_force_mask():
    from deep_calcium_amd.motion import valid_rectangle
    shape = (30, 41)
    rs = np.random.RandomState(4)
    cases = [('rigid', rs.randint(-5, 6, size=(7, 2)), False), ('rigid one-sided', rs.randint(1, 6, size=(5, 2)), False),
             ('rigid other side', -rs.randint(1, 6, size=(5, 2)), False), ('block', rs.randint(-4, 5, size=(3, 2, 3, 2)), False),
             ('fine', rs.randint(-70, 71, size=(7, 2)), True), ('fine whole', 16 * rs.randint(-3, 4, size=(4, 2)), True),
             ('fine block', rs.randint(-50, 51, size=(2, 2, 2, 2)), True), ('none', None, False), ('none fine', None, True)]
    for name, shifts, fine in cases:
        for p in (0, 1, -1, 4, -4, 9, -9):
            want = _brute(shifts, shape, p, fine)
            got = valid_rectangle(shifts, shape, fine=fine, bidi=p)
            assert got == want, (name, p, got, want)
            xs = None if shifts is None else np.asarray(shifts)[..., 1]
            assert got[1] == bref.valid_columns(xs, shape[1], p, fine)
            if p == 0 and shifts is not None:
                assert got == valid_rectangle(shifts, shape, fine=fine)      # the default: nothing differs
    assert valid_rectangle(None, shape, bidi=3) == ((0, 30), (0, 38)) and valid_rectangle(None, shape, bidi=-3) == ((0, 30), (3, 41))
    assert valid_rectangle(np.zeros((0, 2), np.int32), shape) == ((0, 30), (0, 41))


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------
def test_oracle_self_checks():
    # one odd row, by hand: rows (1 2 3 4 5), (10 20 30 40 50), (0 0 0 0 0), P = 1, interior x = 1, 2, 3
    f = np.array([[[1, 2, 3, 4, 5], [10, 20, 30, 40, 50], [0, 0, 0, 0, 0]]], np.int16)
    want = [sum((2 * f[0, 1, x + p] - f[0, 0, x]) ** 2 for x in (1, 2, 3)) for p in (-1, 0, 1)]
    assert bref.scores(f, 1).tolist() == [want]
    assert bref.scores(np.concatenate([f, f[:, 1:2]], axis=1), 1).tolist() == [want]        # H = 4: y = 3 has no line below it and is dropped
    # a vertical ramp costs nothing at any offset; a constant frame neither
    ramp = np.repeat(np.arange(9, dtype=np.int16)[:, None] * 100, 12, axis=1)[None]
    assert (bref.scores(ramp, 3) == 0).all() and (bref.scores(np.full((2, 5, 9), -7, np.int16), 2) == 0).all()
    # the extreme frame: e = +-131070
    for dtype in (np.int16, np.uint16):
        info = np.iinfo(dtype)
        g = np.empty((1, 3, 1), dtype)
        g[0, 0::2], g[0, 1] = info.max, info.min
        assert bref.scores(g, 0).tolist() == [[131070 ** 2]]
    # apply: the convention, both signs, fill by its bits, |p| >= W
    a = np.arange(24, dtype=np.int16).reshape(1, 4, 6)
    assert bref.apply(a, 2, -1)[0].tolist() == [[0, 1, 2, 3, 4, 5], [8, 9, 10, 11, -1, -1], [12, 13, 14, 15, 16, 17], [20, 21, 22, 23, -1, -1]]
    assert bref.apply(a, -1, 9)[0, 1].tolist() == [9, 6, 7, 8, 9, 10] and np.array_equal(bref.apply(a, 0, 5), a)
    assert (bref.apply(a.astype(np.uint16), 6, 65535)[0, 1::2] == 65535).all() and (bref.apply(a, -6, 65535)[0, 1::2] == -1).all()
    # found as p = -b: moving the planted frames by the pick undoes the cut wherever the row is covered
    fr = bref.planted(0, 16, 24, 3, 6, 0, 1, 2)
    p = bref.pick(bref.totals(bref.scores(fr, 3)))
    clean = bref.planted(0, 16, 24, 3, 6, 0, 1, 0)
    assert p == -2 and np.array_equal(bref.apply(fr, p, 0)[:, :, 2:], clean[:, :, 2:])


@pytest.mark.parametrize('config', bref.CONFIGS, ids=lambda c: 'x'.join(str(v) for v in c))
def test_the_oracle_recovers_every_planted_offset(config):
    H, W, P, blobs, sigma, n, seeds = config
    for seed in range(seeds):
        for b in range(-P + 1, P):
            frames = bref.planted(seed, H, W, P, blobs, sigma, n, b)
            assert frames.shape == (n, H, W) and frames.dtype == np.int16
            assert bref.pick(bref.totals(bref.scores(frames, P))) == -b, (seed, b)


def test_summing_over_frames_is_what_recovers_the_noisy_recording():
    H, W, P, blobs, sigma, n, seeds = bref.NOISY
    single_misses = picks = 0
    for seed in range(seeds):
        for b in range(-P + 1, P):
            sc = bref.scores(bref.planted(seed, H, W, P, blobs, sigma, n, b), P)
            assert bref.pick(bref.totals(sc)) == -b, (seed, b)
            single_misses += sum(bref.pick(row.tolist()) != -b for row in sc)
            picks += len(sc)
    assert picks == 480 and single_misses >= 1                              # per-frame picks alone would not pass


def test_frames_of_one_call_are_limited(dclib):
    """DC_FRAMES_PER_CALL_MAX: tc = 2^30 + 1 is refused with (-3) and the limit's message before any launch, tc = 2^30 is not."""
    import _wideindex
    _wideindex.check_frame_limit(dclib, 'test_bidi_api')
