"""The wide (coarse-to-fine) shift search without a GPU: the header constants and the ABI of the three new entry points, argument
validation in front of and inside the library, the oracle's own properties, and the new arithmetic of csrc/motion_math.h as a
stand-alone program under the host sanitizers."""
import inspect
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _motion_ref as ref
import _motion_wide_ref as wref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _boom(*a, **k):
    raise AssertionError('the library was touched')


def test_abi_of_the_new_entry_points():
    from deep_calcium_amd import _gen_tape, _lib, motion
    protos = _lib.parse_header()
    tapeable = dict(_gen_tape.prototypes())
    want = {'dc_motion_bin': ['frames', 'is_unsigned', 'tc', 'H', 'W', 'c', 'out', 'stream'],
            'dc_motion_ssd_around': ['frames', 'is_unsigned', 'tc', 'tmpl', 'H', 'W', 'S', 'D', 'rows', 'mult', 'wscores', 'stream'],
            'dc_motion_pick_around': ['wscores', 'rows', 'mult', 'tc', 'S', 'D', 'shifts', 'best', 'fine', 'stream']}
    for name, args in want.items():
        assert name in protos and name in tapeable, name
        assert protos[name][2] == args and len(tapeable[name]) == len(args)
    assert open(_gen_tape.OUT).read() == _gen_tape.render()
    header = open(_lib.HEADER).read()
    math_h = open(os.path.join(ROOT, 'deep_calcium_amd', 'csrc', 'motion_math.h')).read()
    assert 'DC_MOTION_MAX_WIDE_SHIFT 128' in header and 'DC_MOTION_MAX_WIDE_SHIFT 128' in math_h
    assert 'DC_MOTION_MAX_SHIFT 16' in header                       # the exhaustive limit stays
    assert motion.MAX_WIDE_SHIFT == 128 == motion.MAX_SHIFT * max(motion.COARSE) and motion.COARSE == (2, 4, 8) and motion.MAX_SHIFT == 16
    assert _lib.header_abi_version() >= 118
    for name in ('coarse_shifts', 'coarse_shifts_device', 'last_coarse_scores'):
        assert callable(getattr(motion.MotionCorrector, name))
    for fn in (motion.MotionCorrector.__init__, motion.make_template, motion.estimate_shifts_device):
        assert inspect.signature(fn).parameters['coarse'].default is None
    # the documents say what the search is not
    for text in (header, motion.__doc__, open(os.path.join(ROOT, 'README.md')).read()):
        assert 'NOT the exhaustive argmin' in text


def test_motion_module_still_imports_without_torch_or_the_library():
    code = ("import sys, deep_calcium_amd.motion as m; "
            "assert 'torch' not in sys.modules and 'deep_calcium_amd._lib' not in sys.modules; print(m.MAX_WIDE_SHIFT, m.COARSE)")
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == '128 (2, 4, 8)', out.stderr[-500:]


def test_coarse_keyword_is_checked_before_the_library_is_touched(monkeypatch):
    from deep_calcium_amd import _lib, motion
    monkeypatch.setattr(_lib, 'lib', _boom)
    M = motion.MotionCorrector
    t = np.zeros((200, 220), np.int16)
    # coarse=None: not a message differs -- max_shift = 17 alone is still the exhaustive search's error
    for kw in ({'max_shift': 17}, {'max_shift': 17, 'coarse': None}, {'max_shift': 48}):
        with pytest.raises(ValueError, match=r'max_shift must be in \[0, 16\], not'):
            M((200, 220), 4, np.int16, t, **kw)
    with pytest.raises(ValueError, match=r'max_shift must be in \[0, 16\]'):
        motion.make_template(np.zeros((3, 200, 220), np.int16), max_shift=17)
    with pytest.raises(ValueError, match=r'max_shift must be in \[0, 16\]'):
        motion.estimate_shifts_device('/nonexistent/dataset.npz', max_shift=17)
    for bad in (0, 1, 3, 5, 16, -2, 2.0, '4', True, (4,)):
        with pytest.raises(ValueError, match='coarse must be None or one of 2, 4, 8'):
            M((200, 220), 4, np.int16, t, max_shift=8, coarse=bad)
        with pytest.raises(ValueError, match='coarse must be None or one of 2, 4, 8'):
            motion.estimate_shifts_device('/nonexistent/dataset.npz', max_shift=8, coarse=bad)
        with pytest.raises(ValueError, match='coarse must be None or one of 2, 4, 8'):
            motion.make_template(np.zeros((3, 200, 220), np.int16), max_shift=8, coarse=bad)
    # with coarse = c, max_shift lies in [c, 16 c]
    for c, S in ((2, 1), (2, 33), (4, 3), (4, 65), (8, 7), (8, 129), (4, 0), (4, -1)):
        with pytest.raises(ValueError, match=r'max_shift must be in \[%d, %d\] with coarse = %d, not %d' % (c, 16 * c, c, S)):
            M((600, 600), 4, np.int16, np.zeros((600, 600), np.int16), max_shift=S, coarse=c)
        with pytest.raises(ValueError, match=r'max_shift must be in \[%d, %d\] with coarse' % (c, 16 * c)):
            motion.estimate_shifts_device('/nonexistent/dataset.npz', max_shift=S, coarse=c)
    with pytest.raises(ValueError, match='max_shift must be an integer.*coarse = 4'):
        M((200, 220), 4, np.int16, t, max_shift=8.0, coarse=4)
    # the frame keeps an interior at both levels, and the message names coarse
    for shape, S, c, what in (((96, 220), 48, 4, r'max_shift = 48 with coarse = 4 leaves no interior in a 96 x 220 frame'),
                              ((200, 64), 32, 2, r'max_shift = 32 with coarse = 2 leaves no interior'),
                              # 99 > 2 * 48, but floor(99 / 8) = 12 bins against a coarse radius of 6
                              ((99, 220), 48, 8, r'coarse = 8 leaves no interior in the binned 12 x 27 frame at the coarse radius 6'),
                              ((200, 67), 33, 4, r'coarse = 4 leaves no interior in the binned 50 x 16 frame at the coarse radius 9')):
        with pytest.raises(ValueError, match=what):
            M(shape, 4, np.int16, np.zeros(shape, np.int16), max_shift=S, coarse=c)
        with pytest.raises(ValueError, match='coarse'):
            motion.make_template(np.zeros((2,) + shape, np.int16), max_shift=S, coarse=c)
    # blocks together with coarse is not built
    with pytest.raises(ValueError, match='blocks together with coarse = 4 is not built'):
        M((200, 220), 4, np.int16, t, max_shift=8, coarse=4, blocks=(2, 2))
    with pytest.raises(ValueError, match='blocks together with coarse = 2 is not built'):
        motion.estimate_shifts_device('/nonexistent/dataset.npz', max_shift=8, coarse=2, blocks=(2, 2))
    # legal values reach the library
    for kw in ({'max_shift': 48, 'coarse': 4}, {'max_shift': 4, 'coarse': 4}, {'max_shift': 32, 'coarse': 2}, {'max_shift': 64, 'coarse': np.int64(8)},
               {'max_shift': 17, 'coarse': 2, 'subpixel': True}):
        with pytest.raises(AssertionError, match='the library was touched'):
            M((200, 220), 4, np.int16, t, **kw)
    # an exhaustive corrector has no coarse shifts
    mc = M.__new__(M)
    mc.coarse = None
    for name in ('coarse_shifts', 'coarse_shifts_device', 'last_coarse_scores'):
        with pytest.raises(ValueError, match='coarse=2, 4 or 8'):
            getattr(mc, name)()


def test_cli_refuses_coarse_without_register_or_with_blocks():
    """`traces ... --register 48 --coarse 4`: the command line itself (a process of its own: the script seeds numpy on import).
    Both errors come before a dataset or the GPU is looked for."""
    script = os.path.join(ROOT, 'examples', 'neurons', 'unet2ds_nf.py')
    base = [sys.executable, script, 'traces', 'nonexistent.hdf5', '-m', 'nonexistent_model.hdf5', '-c', '/nonexistent']
    for extra, what in ((['--coarse', '4'], '--coarse needs --register'),
                        (['--register', '48', '--coarse', '4', '--blocks', '2x2'], '--coarse together with --blocks is not built'),
                        (['--register', '48', '--coarse', '3'], 'invalid choice')):
        out = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert out.returncode != 0 and what in out.stderr, (extra, out.stderr[-500:])


def test_c_abi_argument_validation_returns_codes(dclib):
    """Refused before any launch (there is no GPU here): the pointers are never followed."""
    from deep_calcium_amd._lib import DcunetError
    p = 4096
    mbin, around, pick = dclib.dc_motion_bin, dclib.dc_motion_ssd_around, dclib.dc_motion_pick_around

    def bin_args(frames=p, uns=0, tc=1, H=40, W=50, c=4, out=16 * p):
        return (frames, uns, tc, H, W, c, out, None)
    for kw in ({'frames': None}, {'out': None}):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            mbin(*bin_args(**kw))
    for kw in ({'tc': -1}, {'H': 0}, {'W': -3}):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative or zero'):
            mbin(*bin_args(**kw))
    for c in (0, 1, 3, 5, 6, 16, -2):
        with pytest.raises(DcunetError, match=r'\(-3\).*limited to 2, 4 and 8'):
            mbin(*bin_args(c=c))
    with pytest.raises(DcunetError, match=r'\(-3\).*2\^30'):
        mbin(*bin_args(H=2 ** 15, W=2 ** 15 + 1))
    for kw in ({'H': 3}, {'W': 3}, {'H': 7, 'c': 8}, {'W': 1, 'c': 2}):
        with pytest.raises(DcunetError, match=r'\(-1\).*holds no'):
            mbin(*bin_args(**kw))
    for kw in ({'frames': p + 1}, {'out': 16 * p + 1}):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            mbin(*bin_args(**kw))
    for kw in ({'out': p}, {'out': p + 2 * 40 * 50 - 2}, {'frames': 16 * p, 'out': 16 * p - 2 * 10 * 12 + 2}, {'tc': 2, 'out': p + 2 * 40 * 50}):
        with pytest.raises(DcunetError, match=r'\(-1\).*out overlaps frames'):
            mbin(*bin_args(**kw))
    assert mbin(*bin_args(tc=0)) == 0 and mbin(*bin_args(tc=0, uns=1, c=8)) == 0

    def around_args(frames=p, uns=0, tc=1, tmpl=p, H=300, W=320, S=48, D=4, rows=p, mult=4, wscores=p):
        return (frames, uns, tc, tmpl, H, W, S, D, rows, mult, wscores, None)
    for kw in ({'frames': None}, {'tmpl': None}, {'rows': None}, {'wscores': None}):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            around(*around_args(**kw))
    for kw in ({'tc': -1}, {'S': -1}, {'D': -1}, {'H': 0}, {'W': 0}):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative or zero'):
            around(*around_args(**kw))
    with pytest.raises(DcunetError, match=r'\(-3\).*limited to 128'):
        around(*around_args(S=129, H=600, W=600))
    with pytest.raises(DcunetError, match=r'\(-3\).*limited to 8'):
        around(*around_args(D=9))
    with pytest.raises(DcunetError, match=r'\(-3\).*2\^30'):
        around(*around_args(H=2 ** 15, W=2 ** 15 + 1))
    with pytest.raises(DcunetError, match=r'\(-1\).*smaller than the window'):
        around(*around_args(S=3, D=4))
    for kw in ({'H': 96}, {'W': 96}, {'H': 256, 'W': 600, 'S': 128, 'D': 8}):
        with pytest.raises(DcunetError, match=r'\(-1\).*no interior'):
            around(*around_args(**kw))
    for kw in ({'frames': p + 1}, {'tmpl': p + 1}, {'rows': p + 2}, {'wscores': p + 4}):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            around(*around_args(**kw))
    assert around(*around_args(tc=0)) == 0 and around(*around_args(tc=0, S=128, D=8, H=257, W=257, mult=8)) == 0
    assert around(*around_args(tc=0, S=4, D=0)) == 0 and around(*around_args(tc=0, mult=-2 ** 31)) == 0

    def pick_args(wscores=p, rows=p, mult=4, tc=1, S=48, D=4, shifts=p, best=None, fine=None):
        return (wscores, rows, mult, tc, S, D, shifts, best, fine, None)
    for kw in ({'wscores': None}, {'rows': None}, {'shifts': None}):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            pick(*pick_args(**kw))
    for kw in ({'tc': -1}, {'S': -1}, {'D': -1}):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
            pick(*pick_args(**kw))
    with pytest.raises(DcunetError, match=r'\(-3\).*limited to 128'):
        pick(*pick_args(S=129))
    with pytest.raises(DcunetError, match=r'\(-3\).*limited to 8'):
        pick(*pick_args(D=9))
    with pytest.raises(DcunetError, match=r'\(-1\).*smaller than the window'):
        pick(*pick_args(S=1, D=2))
    for kw in ({'wscores': p + 4}, {'rows': p + 2}, {'shifts': p + 2}, {'best': p + 4}, {'fine': p + 2}):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            pick(*pick_args(**kw))
    assert pick(*pick_args(tc=0)) == 0 and pick(*pick_args(tc=0, best=p, fine=p)) == 0       # best and fine are nullable
    # the exhaustive entry points keep their limit and their message
    with pytest.raises(DcunetError, match=r'\(-3\).*search radius is limited to 16'):
        dclib.dc_motion_ssd(p, 0, 1, p, 400, 500, 17, p, None)
    with pytest.raises(DcunetError, match=r'\(-3\).*search radius is limited to 16'):
        dclib.dc_motion_pick(p, 1, 17, p, None, None)


def test_oracle_self_checks():
    # bin: the floor for a negative sum; a constant cell keeps its value at the extremes of both dtypes
    assert wref.bin_frames(np.array([[[-1, -1], [-1, -2]]], np.int16), 2).tolist() == [[[-1]]]
    assert wref.bin_frames(np.array([[[-1, -2], [-2, -2]]], np.int16), 2).tolist() == [[[-2]]]       # -7/4 = -1.75 -> -2
    assert wref.bin_frames(np.array([[[1, 2], [2, 1]]], np.int16), 2).tolist() == [[[2]]]            # 1.5 rounds up
    assert wref.bin_frames(np.array([[[-1, -2], [-2, -1]]], np.int16), 2).tolist() == [[[-1]]]       # -1.5 rounds up
    for dtype in (np.int16, np.uint16):
        info = np.iinfo(dtype)
        for v in (info.min, info.max):
            for c in (2, 4, 8):
                out = wref.bin_frames(np.full((2, 17, 19), v, dtype), c)
                assert out.dtype == dtype and out.shape == (2, 17 // c, 19 // c) and (out == v).all()
        rs = np.random.RandomState(3)
        f = rs.randint(info.min, info.max + 1, size=(2, 9, 11)).astype(dtype)
        b = wref.bin_frames(f, 2)
        assert b.shape == (2, 4, 5)                                  # the trailing row and column are dropped
        cells = f[:, :8, :10].astype(np.int64).reshape(2, 4, 2, 5, 2)
        assert (b >= cells.min(axis=(2, 4))).all() and (b <= cells.max(axis=(2, 4))).all()
        assert np.array_equal(wref.bin_frames(f[0], 2), b[0])        # a template is binned by the same function
    # centre: clamped at +-(S - D), the product beyond int32
    assert wref.centres([[3, -6], [5, 0], [2 ** 31 - 1, -2 ** 31]], 4, 24, 4).tolist() == [[12, -20], [20, 0], [20, -20]]
    assert wref.centres([[1, 1]], 8, 8, 8).tolist() == [[0, 0]]
    # pick: centre (4, 0), D = 2, equal minima at the residuals (-2, 0) and (1, 0): the total shifts (2, 0) and (5, 0)
    w = np.full((1, 5, 5), 100, np.int64)
    w[0, 0, 2] = w[0, 3, 2] = 7
    shifts, best, fine = wref.pick_around(w, [[1, 0]], 4, 6)
    assert shifts.tolist() == [[2, 0]] and best.tolist() == [7]
    assert (ref.pick(w) + [[4, 0]]).tolist() == [[5, 0]]             # what an order over the residuals would give
    assert fine.tolist() == [[32, 0]]                                # the residual (-2, 0) lies on the window's border: q = 0 on y
    # a constant window: the candidate of smallest total displacement
    shifts, _, fine = wref.pick_around(np.full((3, 5, 5), 9, np.int64), [[1, 0], [-3, 2], [0, 0]], 4, 20)
    assert shifts.tolist() == [[2, 0], [-10, 6], [0, 0]] and np.array_equal(fine, 16 * shifts)
    # the window table is the matching sub-block of the exhaustive table
    rs = np.random.RandomState(9)
    tmpl = rs.randint(-3000, 3000, size=(30, 34)).astype(np.int16)
    frames = rs.randint(-3000, 3000, size=(4, 30, 34)).astype(np.int16)
    S, D = 6, 2
    full = ref.scores(frames, tmpl, S)
    rows = np.array([[2, -2], [0, 0], [-1, 1], [100, -100]])
    ctr = wref.centres(rows, 2, S, D)
    assert ctr.tolist() == [[4, -4], [0, 0], [-2, 2], [4, -4]]
    ws = wref.window_scores(frames, tmpl, S, D, rows, 2)
    for k in range(4):
        cy, cx = ctr[k]
        assert np.array_equal(ws[k], full[k, S + cy - D:S + cy + D + 1, S + cx - D:S + cx + D + 1])
    # whenever the exhaustive pick lies in the window, the wide pick is the exhaustive pick
    pk = ref.pick(full)
    got, _, _ = wref.pick_around(wref.window_scores(frames, tmpl, S, D, pk, 1), pk, 1, S)
    assert np.array_equal(got, pk)


@pytest.mark.parametrize('dtype', [np.int16, np.uint16])
@pytest.mark.parametrize('H,W,S,c', [(96, 112, 24, 4), (64, 80, 20, 2), (160, 176, 32, 8)])
def test_the_oracle_recovers_the_planted_offsets(H, W, S, c, dtype):
    tmpl, frames, offsets = wref.planted(H, W, S, c, dtype)
    assert len(offsets) == 32 and np.abs(offsets).max() == S
    r = wref.search(frames, tmpl, S, c)
    assert np.array_equal(r['shifts'], -offsets)
    assert (r['best'] == 0).all()


def test_the_search_is_not_the_exhaustive_argmin():
    """What the documents state plainly: at 40 x 44, S = 8, c = 4 the coarse interior is 6 x 7 bins, the coarse pick of one of the
    32 planted frames lands elsewhere, and the window misses the offset the exhaustive search finds."""
    tmpl, frames, offsets = wref.planted(40, 44, 8, 4, np.int16)
    r = wref.search(frames, tmpl, 8, 4)
    full = ref.pick(ref.scores(frames, tmpl, 8))
    assert np.array_equal(full, -offsets)
    missed = (r['shifts'] != full).any(axis=1)
    assert missed.sum() == 1
    ctr = wref.centres(r['coarse'], 4, 8, 4)
    assert (np.abs(full - ctr).max(axis=1) > 4)[missed].all() and (np.abs(full - ctr).max(axis=1) <= 4)[~missed].all()


@pytest.mark.parametrize('dtype', [np.int16, np.uint16])
def test_the_oracle_at_coarse_2_agrees_with_the_exhaustive_search(dtype):
    H, W, S, c = 48, 52, 16, 2
    tmpl, frames, offsets = wref.planted(H, W, S, c, dtype)
    r = wref.search(frames, tmpl, S, c)
    assert np.array_equal(r['shifts'], ref.pick(ref.scores(frames, tmpl, S))) and np.array_equal(r['shifts'], -offsets)


def test_arithmetic_under_the_host_sanitizers(tmp_path):
    """The wide-search arithmetic of csrc/motion_math.h -- the rounding rule of the bin (the floor for negative sums), the centre
    clamp with mult * row beyond int32, the order over total shifts against a brute-force tuple comparison -- compiled into
    tests/native/motion_wide_check.cpp with the address and undefined-behaviour sanitizers and run as a program of its own."""
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
    exe = str(tmp_path / 'motion_wide_check')
    src = os.path.join(ROOT, 'tests', 'native', 'motion_wide_check.cpp')
    r = subprocess.run([cxx] + flags + [src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'motion_wide_check: ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_frames_of_one_call_are_limited(dclib):
    """DC_FRAMES_PER_CALL_MAX: tc = 2^30 + 1 is refused with (-3) and the limit's message before any launch, tc = 2^30 is not."""
    import _wideindex
    _wideindex.check_frame_limit(dclib, 'test_motion_wide_api')
