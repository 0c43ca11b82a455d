"""Sub-pixel motion correction without a GPU: argument validation in front of and inside the library, the ABI of the four new
entry points, the host helpers, the oracle's own properties, and the arithmetic of csrc/motion_math.h as a stand-alone program
under the host sanitizers."""
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import _motion_block_ref as bref
import _motion_ref as ref
import _motion_sub_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _boom(*a, **k):
    raise AssertionError('the library was touched')


def test_subpixel_keyword_is_checked_before_the_library_is_touched(monkeypatch):
    from deep_calcium_amd import _lib, motion
    monkeypatch.setattr(_lib, 'lib', _boom)
    t16 = np.zeros((40, 50), np.int16)
    M = motion.MotionCorrector
    for bad in (1, 0, 'yes', None, 1.0, (True,)):
        with pytest.raises(ValueError, match='subpixel must be True or False'):
            M((40, 50), 4, np.int16, t16, subpixel=bad)
        with pytest.raises(ValueError, match='subpixel must be True or False'):
            M((70, 120), 4, np.int16, np.zeros((70, 120), np.int16), blocks=(2, 3), subpixel=bad)
        with pytest.raises(ValueError, match='subpixel must be True or False'):
            motion.estimate_shifts_device('/nonexistent/dataset.npz', subpixel=bad)
    # a legal value reaches the library, and the default is the whole-pixel corrector
    for kw in ({'subpixel': True}, {'subpixel': False}, {'subpixel': np.True_}, {}):
        with pytest.raises(AssertionError, match='the library was touched'):
            M((40, 50), 4, np.int16, t16, **kw)
    for fn in (M.__init__, motion.estimate_shifts_device):
        assert inspect.signature(fn).parameters['subpixel'].default is False
    assert inspect.signature(motion.valid_rectangle).parameters['fine'].default is False
    # a whole-pixel corrector has no fine shifts
    mc = M.__new__(M)
    mc.subpixel = False
    for name in ('fine_shifts', 'fine_shifts_device'):
        with pytest.raises(ValueError, match='subpixel=True'):
            getattr(mc, name)()


def test_fine_shifts_keyword_is_checked_before_the_library_is_touched(monkeypatch):
    from deep_calcium_amd import _lib, series, traces
    monkeypatch.setattr(_lib, 'lib', _boom)
    ok = [np.array([[1, 2], [3, 4]])]
    for bad in (np.zeros((5, 2), np.int32), np.zeros((4, 3), np.int32), np.zeros((4,), np.int32),      # rigid: wrong shape
                np.zeros((4, 2), np.float32), np.zeros((4, 2), np.float64), np.zeros((4, 2), bool),      # wrong dtype
                np.full((4, 2), 2 ** 31, np.int64),
                np.zeros((5, 2, 2, 2), np.int32), np.zeros((4, 2, 2, 3), np.int32), np.zeros((4, 2, 2), np.int32),
                np.zeros((4, 0, 2, 2), np.int32), np.zeros((4, 33, 1, 2), np.int32),
                np.zeros((4, 6, 1, 2), np.int32),              # more blocks than the 5 rows of the frame
                np.zeros((4, 2, 2, 2), np.float32)):
        with pytest.raises(ValueError, match='fine_shifts must'):
            series.SeriesSummarizer((5, 7), 4, np.int16, fine_shifts=bad)
        with pytest.raises(ValueError, match='fine_shifts must'):
            traces.RoiTraceExtractor((5, 7), 4, np.int16, ok, fine_shifts=bad)
    good, fine = np.zeros((4, 2), np.int32), np.zeros((4, 2, 3, 2), np.int64)
    for kw in ({'shifts': good, 'fine_shifts': good}, {'shifts': good, 'fine_shifts': fine}, {'shifts': fine, 'fine_shifts': good}):
        with pytest.raises(ValueError, match='not both'):
            series.SeriesSummarizer((5, 7), 4, np.int16, **kw)
        with pytest.raises(ValueError, match='not both'):
            traces.RoiTraceExtractor((5, 7), 4, np.int16, ok, **kw)
        with pytest.raises(ValueError, match='not both'):                 # before the file is looked for
            series.summarize_series_device('/nonexistent/dataset.npz', **kw)
        with pytest.raises(ValueError, match='not both'):
            traces.extract_traces_device('/nonexistent/dataset.npz', ok, **kw)
    # shifts= keeps rejecting floating arrays, under its own name
    with pytest.raises(ValueError, match='^shifts must'):
        series.SeriesSummarizer((5, 7), 4, np.int16, shifts=np.zeros((4, 2), np.float32))
    # a legal table reaches the library
    for kw in ({'fine_shifts': good}, {'fine_shifts': fine}, {'fine_shifts': [[-17, 40]] * 4}):
        with pytest.raises(AssertionError, match='the library was touched'):
            series.SeriesSummarizer((5, 7), 4, np.int16, **kw)
        with pytest.raises(AssertionError, match='the library was touched'):
            traces.RoiTraceExtractor((5, 7), 4, np.int16, ok, **kw)
    for fn in (series.SeriesSummarizer.__init__, traces.RoiTraceExtractor.__init__, series.summarize_series_device,
               traces.extract_traces_device):
        assert inspect.signature(fn).parameters['fine_shifts'].default is None


def test_abi_of_the_new_entry_points():
    import deep_calcium_amd
    from deep_calcium_amd import _gen_tape, _lib, motion
    protos = _lib.parse_header()
    tapeable = dict(_gen_tape.prototypes())
    want = {'dc_motion_refine': ['scores', 'shifts', 'tc', 'S', 'fine', 'stream'],
            'dc_motion_block_refine': ['bscores', 'rigid', 'block_shifts', 'tc', 'By', 'Bx', 'S', 'D', 'fine', 'stream'],
            'dc_motion_apply_sub': ['frames', 'is_unsigned', 'tc', 'fine', 'H', 'W', 'fill', 'out', 'stream'],
            'dc_motion_warp_sub': ['frames', 'is_unsigned', 'tc', 'fine_block_shifts', 'By', 'Bx', 'H', 'W', 'fill', 'out', 'stream']}
    for name, args in want.items():
        assert name in protos and name in tapeable, name
        assert protos[name][2] == args and len(tapeable[name]) == len(args)
    assert open(_gen_tape.OUT).read() == _gen_tape.render()
    header = open(_lib.HEADER).read()
    assert 'DC_MOTION_SUB 16' in header and motion.SUBPIXEL == 16 == sref.Q
    assert 'DC_MOTION_SUB 16' in open(os.path.join(ROOT, 'deep_calcium_amd', 'csrc', 'motion_math.h')).read()
    assert _lib.header_abi_version() >= 115
    assert deep_calcium_amd.fine_to_pixels is motion.fine_to_pixels and 'fine_to_pixels' in deep_calcium_amd.__all__
    for name in ('fine_shifts', 'fine_shifts_device'):
        assert callable(getattr(motion.MotionCorrector, name))


def test_c_abi_argument_validation_returns_codes(dclib):
    """Refused before any launch (there is no GPU here): the pointers are never followed."""
    from deep_calcium_amd._lib import DcunetError
    p = 4096
    refine, brefine, apply_sub, warp_sub = (dclib.dc_motion_refine, dclib.dc_motion_block_refine, dclib.dc_motion_apply_sub,
                                            dclib.dc_motion_warp_sub)

    def refine_args(scores=p, shifts=p, tc=1, S=8, fine=p):
        return (scores, shifts, tc, S, fine, None)
    for kw in ({'scores': None}, {'shifts': None}, {'fine': None}):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            refine(*refine_args(**kw))
    for kw in ({'tc': -1}, {'S': -1}):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
            refine(*refine_args(**kw))
    with pytest.raises(DcunetError, match=r'\(-3\).*limited to 16'):
        refine(*refine_args(S=17))
    for kw in ({'scores': p + 4}, {'shifts': p + 2}, {'fine': p + 2}):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            refine(*refine_args(**kw))
    assert refine(*refine_args(tc=0)) == 0 and refine(*refine_args(tc=0, S=16)) == 0

    def brefine_args(bscores=p, rigid=p, block_shifts=p, tc=1, By=2, Bx=3, S=8, D=3, fine=p):
        return (bscores, rigid, block_shifts, tc, By, Bx, S, D, fine, None)
    for kw in ({'bscores': None}, {'rigid': None}, {'block_shifts': None}, {'fine': None}):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            brefine(*brefine_args(**kw))
    for kw in ({'tc': -1}, {'S': -1}, {'D': -1}, {'By': 0}, {'Bx': 0}):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative or zero'):
            brefine(*brefine_args(**kw))
    for kw, what in (({'S': 17}, 'limited to 16'), ({'D': 9}, 'limited to 8'), ({'By': 33}, 'limited to 32 x 32')):
        with pytest.raises(DcunetError, match=r'\(-3\).*' + what):
            brefine(*brefine_args(**kw))
    for kw in ({'bscores': p + 4}, {'rigid': p + 2}, {'block_shifts': p + 2}, {'fine': p + 2}):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            brefine(*brefine_args(**kw))
    assert brefine(*brefine_args(tc=0)) == 0

    def apply_args(frames=p, uns=0, tc=1, fine=p, H=40, W=50, fill=0, out=2 * p):
        return (frames, uns, tc, fine, H, W, fill, out, None)

    def warp_args(frames=p, uns=0, tc=1, fine=p, By=2, Bx=3, H=40, W=50, fill=0, out=2 * p):
        return (frames, uns, tc, fine, By, Bx, H, W, fill, out, None)
    for fn, args in ((apply_sub, apply_args), (warp_sub, warp_args)):
        for kw in ({'frames': None}, {'fine': None}, {'out': None}):
            with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
                fn(*args(**kw))
        for kw in ({'tc': -1}, {'H': 0}, {'W': -1}):
            with pytest.raises(DcunetError, match=r'\(-1\).*negative or zero'):
                fn(*args(**kw))
        with pytest.raises(DcunetError, match=r'\(-3\).*2\^30'):
            fn(*args(H=2 ** 15, W=2 ** 15 + 1))
        for fill in (65536, -32769):
            with pytest.raises(DcunetError, match=r'\(-1\).*fill = %d' % fill):
                fn(*args(fill=fill))
        for kw in ({'frames': p + 1}, {'out': 2 * p + 1}, {'fine': p + 2}):
            with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
                fn(*args(**kw))
        for kw in ({'out': p}, {'tc': 2, 'out': p + 2 * 40 * 50}, {'tc': 2, 'frames': 2 * p, 'out': 2 * p - 2 * 40 * 50}):
            with pytest.raises(DcunetError, match=r'\(-1\).*out overlaps frames'):
                fn(*args(**kw))
        assert fn(*args(tc=0)) == 0 and fn(*args(tc=0, uns=1, fill=65535)) == 0
    for kw in ({'By': 0}, {'Bx': 0}):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative or zero'):
            warp_sub(*warp_args(**kw))
    for kw in ({'By': 33}, {'Bx': 33}):
        with pytest.raises(DcunetError, match=r'\(-3\).*limited to 32 x 32'):
            warp_sub(*warp_args(**kw))
    for kw in ({'H': 3, 'By': 4}, {'W': 2, 'Bx': 3}):
        with pytest.raises(DcunetError, match=r'\(-1\).*a block is empty'):
            warp_sub(*warp_args(**kw))


def test_host_helpers():
    from deep_calcium_amd import fine_to_pixels, valid_rectangle
    H, W = 40, 50
    # hand-made: floor of the smallest and ceiling of the largest sixteenth, for either sign
    for fine, want in (([[0, 0]], ((0, 40), (0, 50))),
                       ([[16, -16]], ((0, 39), (1, 50))),
                       ([[1, -1]], ((0, 39), (1, 50))),                     # a sixteenth costs a whole row: the i = 1 tap is used
                       ([[-1, 1]], ((1, 40), (0, 49))),
                       ([[-17, 33], [15, -32]], ((2, 39), (2, 47))),
                       ([[-16, 16], [-15, 17]], ((1, 40), (0, 48))),
                       ([[-48, -48], [-33, -47]], ((3, 40), (3, 50)))):
        assert valid_rectangle(np.array(fine), (H, W), fine=True) == want == sref.valid_fine(fine, (H, W)), fine
    rs = np.random.RandomState(5)
    for _ in range(50):
        fine = rs.randint(-70, 71, size=(6, 2, 3, 2))
        assert valid_rectangle(fine, (H, W), fine=True) == sref.valid_fine(fine, (H, W))
        whole = 16 * rs.randint(-4, 5, size=(6, 2))                       # multiples of 16: the whole-pixel rule
        assert valid_rectangle(whole, (H, W), fine=True) == valid_rectangle(whole // 16, (H, W)) == ref.valid(whole // 16, (H, W))
    assert valid_rectangle(np.zeros((0, 2), np.int32), (H, W), fine=True) == ((0, H), (0, W))
    assert valid_rectangle(np.array([[3, -2]]), (H, W)) == valid_rectangle(np.array([[3, -2]]), (H, W), fine=False) == ((0, 37), (2, 50))
    with pytest.raises(ValueError, match='fine must be True or False'):
        valid_rectangle(np.array([[3, -2]]), (H, W), fine=1)
    # inside the fine rectangle no pixel of the oracle's interpolation is fill, and the rectangle is tight
    frames = rs.randint(1, 1000, size=(4, 20, 24)).astype(np.int16)
    fine = np.array([[-17, 33], [15, -32], [0, 1], [-1, 0]])
    (y0, y1), (x0, x1) = valid_rectangle(fine, (20, 24), fine=True)
    out = sref.apply_sub(frames, fine, fill=-7)
    assert (out[:, y0:y1, x0:x1] != -7).all()
    for sl in ((slice(None), y0 - 1), (slice(None), y1), (slice(None), slice(None), x0 - 1), (slice(None), slice(None), x1)):
        assert (out[sl] == -7).any()
    got = fine_to_pixels(np.array([[-1, 8], [-40, 17]], np.int32))
    assert got.dtype == np.float64 and got.tolist() == [[-0.0625, 0.5], [-2.5, 1.0625]]
    assert fine_to_pixels([[[[16, -16]]]]).tolist() == [[[[1.0, -1.0]]]]
    with pytest.raises(ValueError, match='integers'):
        fine_to_pixels(np.array([0.5]))


def test_reference_properties():
    rs = np.random.RandomState(11)
    # q in [-8, 8], mirror symmetry, flat and symmetric neighbourhoods, the named values
    for _ in range(3000):
        bits = rs.randint(1, 63)
        s0, a, b = (int(rs.randint(0, 2 ** 31)) * int(rs.randint(0, 2 ** 31)) % (1 << bits) for _ in range(3))
        sm, sp = s0 + a, s0 + b
        q = sref.refine_q(sm, s0, sp)
        assert -8 <= q <= 8 and sref.refine_q(sp, s0, sm) == -q
        assert sref.refine_q(sm, s0, sm) == 0 and sref.refine_q(s0, s0, s0) == 0
        if b > 0:
            assert sref.refine_q(s0, s0, sp) == -8 and sref.refine_q(sp, s0, s0) == 8
    top = 2 ** 62 - 1
    assert sref.refine_q(top, 0, top) == 0 and sref.refine_q(0, 0, top) == -8 and sref.refine_q(top, 0, 0) == 8
    # the tie at half a sixteenth goes to the pick: N / D = 1 / 16, which three scores first give as N = 2, D = 32 (N and D have
    # the same parity); the tie at 1.5 sixteenths goes to 1
    assert sref.refine_q(17, 0, 15) == 0 and sref.refine_q(15, 0, 17) == 0 and sref.refine_q(19, 0, 13) == 1
    assert sref.refine_q(10, 1, 9) == 0 and sref.refine_q(11, 1, 8) == 1             # D = 17: just below and just beyond a half
    assert sref.refine_q(16, 0, 0) == 8 and sref.refine_q(12, 0, 4) == 4              # N / 2D = 1/2 and 1/4 of a pixel
    # a table: a border pick gives 0 on that axis, its mirror image the mirrored q
    for S in (0, 1, 3):
        nd = 2 * S + 1
        sc = rs.randint(100, 10 ** 6, size=(40, nd, nd)).astype(np.int64)
        pk = ref.pick(sc)
        fine = sref.refine(sc, pk)
        q = fine - 16 * pk
        assert np.abs(q).max() <= 8
        assert (q[np.abs(pk) == S] == 0).all()
        assert np.array_equal(sref.refine(sc[:, ::-1, ::-1], -pk), -fine)
        assert np.array_equal(sref.refine(sc, pk + 100), 16 * (pk + 100))             # outside the table: nothing read, q = 0
    # the split
    for s, want in ((0, (0, 0)), (-1, (-1, 15)), (-16, (-1, 0)), (-17, (-2, 15)), (15, (0, 15)), (16, (1, 0)), (-2 ** 31, (-2 ** 27, 0))):
        assert sref.split(s) == want
    # integer fine shifts reproduce _motion_ref's apply, and the whole-pixel field _motion_block_ref's warp
    for dtype, fill in ((np.int16, -2), (np.uint16, 48879)):
        info = np.iinfo(dtype)
        frames = rs.randint(info.min, info.max + 1, size=(6, 9, 11)).astype(dtype)
        shifts = np.array([(0, 0), (2, -3), (-9, 1), (1, 11), (-1, 0), (8, 10)])
        assert np.array_equal(sref.apply_sub(frames, 16 * shifts, fill), ref.apply(frames, shifts, fill))
        bs = np.broadcast_to(shifts[:, None, None, :], (6, 2, 3, 2))
        assert np.array_equal(sref.warp_sub(frames, 16 * bs, fill), bref.warp(frames, bs, fill))
        # equal fine block shifts are apply_sub
        fine = np.array([(1, -1), (-15, 15), (17, -17), (-1, 15), (8, 8), (-40, 23)])
        fbs = np.broadcast_to(fine[:, None, None, :], (6, 2, 3, 2))
        assert np.array_equal(sref.warp_sub(frames, fbs, fill), sref.apply_sub(frames, fine, fill))
        # the result lies between the taps: constant frames stay constant at fractional shifts
        for v in (info.min, info.max):
            const = np.full((1, 9, 11), v, dtype)
            out = sref.apply_sub(const, [(7, -9)], fill)
            assert (out[0, 1:8, 1:10] == v).all() and (out[0, -1] == np.array(fill).astype(dtype)).all()
    # where the fine field of whole-pixel block shifts is itself whole, it is the whole-pixel field
    bs = rs.randint(-3, 4, size=(3, 4, 2))
    f16, f1 = sref.fine_field(16 * bs, 30, 40), bref.field(bs.tolist(), 30, 40)
    whole = (f16 % 16 == 0).all(-1)
    assert whole.any() and not whole.all() and np.array_equal(f16[whole], 16 * f1[whole])


def test_arithmetic_under_the_host_sanitizers(tmp_path):
    """The sub-pixel arithmetic of csrc/motion_math.h compiled into tests/native/motion_sub_check.cpp with the address and
    undefined-behaviour sanitizers and run as a program of its own, against a brute-force restatement in 128-bit integers: scores
    up to 2^62 - 1, the split at the int32 extremes, the interpolation at the int16 and uint16 extremes."""
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
    exe = str(tmp_path / 'motion_sub_check')
    src = os.path.join(ROOT, 'tests', 'native', 'motion_sub_check.cpp')
    r = subprocess.run([cxx] + flags + [src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'motion_sub_check: ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_frames_of_one_call_are_limited(dclib):
    """DC_FRAMES_PER_CALL_MAX: tc = 2^30 + 1 is refused with (-3) and the limit's message before any launch, tc = 2^30 is not."""
    import _wideindex
    _wideindex.check_frame_limit(dclib, 'test_motion_sub_api')
