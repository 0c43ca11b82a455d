"""Piecewise-rigid motion correction without a GPU: the public names and the ABI, argument validation in front of and inside the
library, the numpy oracle's own identities, the valid rectangle on block shifts, and the geometry / field arithmetic of
csrc/motion_math.h as a stand-alone program under the host sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import _motion_block_ref as bref
import _motion_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_public_names_and_abi():
    from deep_calcium_amd import _build, _gen_tape, _lib, motion
    assert _lib.header_abi_version() >= 113 and 'motion.hip' in _build.SOURCES
    protos = _lib.parse_header()
    tapeable = set(n for n, _ in _gen_tape.prototypes())
    want = {'dc_motion_block_ssd': ['frames', 'is_unsigned', 'tc', 'tmpl', 'H', 'W', 'S', 'D', 'By', 'Bx', 'rigid', 'bscores', 'stream'],
            'dc_motion_block_pick': ['bscores', 'rigid', 'tc', 'By', 'Bx', 'S', 'D', 'block_shifts', 'best', 'stream'],
            'dc_motion_warp': ['frames', 'tc', 'block_shifts', 'By', 'Bx', 'H', 'W', 'fill', 'out', 'stream']}
    for name, args in want.items():
        assert name in protos and name in tapeable, name
        assert protos[name][2] == args
    header = open(_lib.HEADER).read()
    assert 'DC_MOTION_MAX_DEV 8' in header and motion.MAX_DEV == 8
    assert 'DC_MOTION_MAX_BLOCKS 32' in header and motion.MAX_BLOCKS == 32
    for text in (header, motion.__doc__, open(os.path.join(ROOT, 'README.md')).read(), open(os.path.join(ROOT, 'DESIGN.md')).read()):
        assert 'piecewise and non-rigid' not in ' '.join(text.split())        # the three "not implemented" sentences are reworded
        assert 'repeated or skipped' in ' '.join(text.split())               # the price of whole-pixel exactness is documented
    import inspect
    for fn in (motion.MotionCorrector.__init__, motion.estimate_shifts_device):
        p = inspect.signature(fn).parameters
        assert p['blocks'].default is None and p['max_dev'].default == 3
    for name in ('block_shifts', 'block_shifts_device', 'last_block_scores'):
        assert callable(getattr(motion.MotionCorrector, name))


def _boom(*a, **k):
    raise AssertionError('the library was touched')


def test_block_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    from deep_calcium_amd import _lib, motion
    monkeypatch.setattr(_lib, 'lib', _boom)
    t16 = np.zeros((40, 50), np.int16)
    M = motion.MotionCorrector
    for kw, what in (({'blocks': 4}, 'blocks must be'),
                     ({'blocks': (4,)}, 'blocks must be'),
                     ({'blocks': (4, 4, 4)}, 'blocks must be'),
                     ({'blocks': (0, 4)}, r'blocks must be .*\[1, 32\]'),
                     ({'blocks': (4, 33)}, r'blocks must be .*\[1, 32\]'),
                     ({'blocks': (2.0, 2)}, 'blocks must be'),
                     ({'blocks': (True, 2)}, 'blocks must be'),
                     ({'blocks': '44'}, 'blocks must be'),
                     ({'blocks': (2, 2), 'max_dev': 9}, r'max_dev must be in \[0, 8\]'),
                     ({'blocks': (2, 2), 'max_dev': -1}, r'max_dev must be in \[0, 8\]'),
                     ({'blocks': (2, 2), 'max_dev': 1.5}, 'max_dev must be an integer'),
                     # 40 rows in 4 blocks of 10: e(1) = 10 is not beyond the margin 8 + 3 = 11
                     ({'blocks': (4, 1), 'max_shift': 8, 'max_dev': 3}, r'blocks = \(4, 1\).*no rows inside the margin max_shift \+ max_dev = 11'),
                     # 50 columns in 5 blocks of 10: e(4) = 40 is not below 50 - 10
                     ({'blocks': (1, 5), 'max_shift': 8, 'max_dev': 2}, r'blocks = \(1, 5\).*no columns'),
                     # one block, but the interior itself is empty: 40 <= 2 * 20
                     ({'blocks': (1, 1), 'max_shift': 16, 'max_dev': 4}, r'blocks = \(1, 1\).*no rows')):
        with pytest.raises(ValueError, match=what):
            M((40, 50), 4, np.int16, t16, **kw)
    # blocks=None: max_dev is not looked at, and the rigid checks are what they were
    with pytest.raises(ValueError, match=r'max_shift must be in \[0, 16\]'):
        M((40, 50), 4, np.int16, t16, max_shift=17, max_dev=99)
    for kw, what in (({'blocks': (0, 1)}, 'blocks must be'), ({'blocks': (2, 2), 'max_dev': 9}, 'max_dev')):
        with pytest.raises(ValueError, match=what):
            motion.estimate_shifts_device('/nonexistent/dataset.npz', **kw)
    # the limits themselves are legal as far as the host checks go (the library is the next thing touched)
    with pytest.raises(AssertionError, match='the library was touched'):
        M((70, 120), 4, np.int16, np.zeros((70, 120), np.int16), max_shift=16, blocks=(2, 3), max_dev=8)
    # a rigid corrector has no block shifts
    mc = M.__new__(M)
    mc.blocks = None
    for name in ('block_shifts', 'block_shifts_device', 'last_block_scores'):
        with pytest.raises(ValueError, match='blocks='):
            getattr(mc, name)()


def test_block_shifts_keyword_is_checked_before_the_library_is_touched(monkeypatch):
    from deep_calcium_amd import _lib, series, traces
    monkeypatch.setattr(_lib, 'lib', _boom)
    ok = [np.array([[1, 2], [3, 4]])]
    for bad in (np.zeros((5, 2, 2, 2), np.int32),              # another number of frames
                np.zeros((4, 2, 2, 3), np.int32),              # not (dy, dx)
                np.zeros((4, 2, 2), np.int32), np.zeros((4, 2, 2, 2, 2), np.int32),
                np.zeros((4, 0, 2, 2), np.int32), np.zeros((4, 33, 1, 2), np.int32), np.zeros((4, 1, 33, 2), np.int32),
                np.zeros((4, 6, 1, 2), np.int32),              # more blocks than the 5 rows of the frame
                np.zeros((4, 1, 8, 2), np.int32),              # ... than its 7 columns
                np.zeros((4, 2, 2, 2), np.float32), np.zeros((4, 2, 2, 2), bool),
                np.full((4, 2, 2, 2), 2 ** 31, np.int64)):
        with pytest.raises(ValueError, match='shifts must'):
            series.SeriesSummarizer((5, 7), 4, np.int16, shifts=bad)
        with pytest.raises(ValueError, match='shifts must'):
            traces.RoiTraceExtractor((5, 7), 4, np.int16, ok, shifts=bad)
    good = series._check_shifts(np.arange(4 * 2 * 3 * 2).reshape(4, 2, 3, 2).astype(np.int64) - 9, 4, (5, 7))
    assert good.dtype == np.int32 and good.shape == (4, 2, 3, 2) and good.flags.c_contiguous
    assert series._check_shifts([[[[1, -2]]]] * 4, 4).shape == (4, 1, 1, 2)
    good = series._check_shifts(np.zeros((4, 32, 32, 2), np.int16), 4)
    assert good.dtype == np.int32
    # a legal array reaches the library
    with pytest.raises(AssertionError, match='the library was touched'):
        series.SeriesSummarizer((5, 7), 4, np.int16, shifts=np.zeros((4, 2, 3, 2), np.int32))


def test_valid_rectangle_on_block_shifts():
    """The field never leaves [min s, max s] of the block shifts, so the rectangle of all block shifts bounds the warped frames."""
    from deep_calcium_amd import valid_rectangle
    rs = np.random.RandomState(3)
    T, H, W, By, Bx = 5, 21, 26, 3, 2
    bs = rs.randint(-4, 5, size=(T, By, Bx, 2)).astype(np.int32)
    rect = valid_rectangle(bs, (H, W))
    assert rect == ref.valid(bs.reshape(-1, 2), (H, W)) == valid_rectangle(bs.reshape(-1, 2), (H, W))
    (y0, y1), (x0, x1) = rect
    assert (y0, x0) == (max(0, -bs[..., 0].min()), max(0, -bs[..., 1].min()))
    frames = rs.randint(1, 1000, size=(T, H, W)).astype(np.int16)          # no pixel equals the fill
    out = bref.warp(frames, bs, fill=-7)
    assert (out[:, y0:y1, x0:x1] != -7).all() and (out == -7).any()
    assert valid_rectangle(np.zeros((0, 2, 2, 2), np.int32), (H, W)) == ((0, H), (0, W))


def test_oracle_identities():
    """What the definitions promise, on the oracle alone: the block scores of a candidate add up to the rigid-style score over the
    margin-M interior; a uniform field is _motion_ref.apply bit for bit; the field stays within the block shifts, int32 extremes
    included."""
    rs = np.random.RandomState(8)
    for H, W, S, D, By, Bx in ((45, 83, 3, 2, 3, 4), (23, 29, 1, 1, 4, 3), (24, 40, 3, 2, 4, 1), (30, 33, 4, 0, 2, 2)):
        M, T = S + D, 3
        assert bref.grid_ok(H, W, By, Bx, M)
        frames = rs.randint(0, 65536, size=(T, H, W)).astype(np.uint16)
        frames[1] = frames[0]
        tmpl = rs.randint(0, 65536, size=(H, W)).astype(np.uint16)
        rigid = np.array([[S, -S], [1000, -1000], [rs.randint(-S, S + 1), rs.randint(-S, S + 1)]])
        bsc = bref.block_scores(frames, tmpl, S, D, By, Bx, rigid)
        assert np.array_equal(bsc[0], bsc[1])                              # the clamp
        full = ref.scores(frames, tmpl, M)                                 # margin M, every shift within +-M
        for t in range(T):
            dy, dx = np.clip(rigid[t], -S, S)
            assert np.array_equal(bsc[t].sum(axis=(0, 1)), full[t, M + dy - D:M + dy + D + 1, M + dx - D:M + dx + D + 1])
    frames = rs.randint(-32768, 32768, size=(4, 9, 11)).astype(np.int16)
    for shift in ((0, 0), (2, -3), (-9, 1), (1, 11), (2 ** 31 - 1, -2 ** 31)):
        bs = np.broadcast_to(np.array(shift, np.int64), (4, 2, 3, 2))
        assert np.array_equal(bref.warp(frames, bs, -2), ref.apply(frames, [shift] * 4, -2))
    bs = np.array([[[2 ** 31 - 1, -2 ** 31], [-2 ** 31, 2 ** 31 - 1]], [[5, -5], [-2 ** 31, 0]]], np.int64)
    f = bref.field(bs.tolist(), 13, 17)
    assert f.min() >= -2 ** 31 and f.max() <= 2 ** 31 - 1 and f[0, 0].tolist() == bs[0, 0].tolist() and f[12, 16].tolist() == bs[1, 1].tolist()
    assert not bref.grid_ok(40, 50, 4, 1, 11) and bref.grid_ok(40, 50, 3, 1, 11) and not bref.grid_ok(40, 50, 1, 1, 20)


def test_c_abi_argument_validation_returns_codes(dclib):
    """Refused before any launch (there is no GPU here): the pointers are never followed."""
    from deep_calcium_amd._lib import DcunetError
    p = 4096                                  # any aligned non-null value
    ssd, pick, warp = dclib.dc_motion_block_ssd, dclib.dc_motion_block_pick, dclib.dc_motion_warp

    def ssd_args(frames=p, tc=1, tmpl=p, H=70, W=120, S=8, D=3, By=2, Bx=3, rigid=p, bscores=p):
        return (frames, 0, tc, tmpl, H, W, S, D, By, Bx, rigid, bscores, None)
    for kw in ({'frames': None}, {'tmpl': None}, {'rigid': None}, {'bscores': None}):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            ssd(*ssd_args(**kw))
    for kw in ({'tc': -1}, {'S': -1}, {'D': -1}, {'H': 0}, {'By': 0}, {'Bx': -2}):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative or zero'):
            ssd(*ssd_args(**kw))
    for kw, what in (({'S': 17}, 'limited to 16'), ({'D': 9}, 'limited to 8'), ({'By': 33}, 'limited to 32 x 32'), ({'Bx': 33}, 'limited to 32 x 32'),
                     ({'H': 2 ** 15, 'W': 2 ** 15 + 1}, r'2\^30')):
        with pytest.raises(DcunetError, match=r'\(-3\).*' + what):
            ssd(*ssd_args(**kw))
    for kw in ({'H': 40, 'W': 50, 'By': 4, 'Bx': 1}, {'H': 40, 'W': 50, 'By': 1, 'Bx': 5, 'D': 2}, {'H': 22, 'W': 50, 'By': 1, 'Bx': 1},
               {'H': 70, 'W': 22, 'By': 1, 'Bx': 1}, {'H': 70, 'W': 120, 'S': 16, 'D': 8, 'By': 3, 'Bx': 3}):
        with pytest.raises(DcunetError, match=r'\(-1\).*no interior'):
            ssd(*ssd_args(**kw))
    for kw in ({'frames': p + 1}, {'tmpl': p + 1}, {'rigid': p + 2}, {'bscores': p + 4}):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            ssd(*ssd_args(**kw))
    assert ssd(*ssd_args(tc=0)) == 0                             # no frames: nothing launched
    assert ssd(*ssd_args(tc=0, H=70, W=120, S=16, D=8, By=2, Bx=3)) == 0      # both radii at their limits are legal

    def pick_args(bscores=p, rigid=p, tc=1, By=2, Bx=3, S=8, D=3, block_shifts=p, best=None):
        return (bscores, rigid, tc, By, Bx, S, D, block_shifts, best, None)
    for kw in ({'bscores': None}, {'rigid': None}, {'block_shifts': None}):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            pick(*pick_args(**kw))
    for kw in ({'tc': -1}, {'S': -1}, {'D': -1}, {'By': 0}, {'Bx': 0}):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative or zero'):
            pick(*pick_args(**kw))
    for kw, what in (({'S': 17}, 'limited to 16'), ({'D': 9}, 'limited to 8'), ({'By': 33}, 'limited to 32 x 32')):
        with pytest.raises(DcunetError, match=r'\(-3\).*' + what):
            pick(*pick_args(**kw))
    for kw in ({'bscores': p + 4}, {'rigid': p + 2}, {'block_shifts': p + 2}, {'best': p + 4}):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            pick(*pick_args(**kw))
    assert pick(*pick_args(tc=0)) == 0 and pick(*pick_args(tc=0, best=p)) == 0

    def warp_args(frames=p, tc=1, block_shifts=p, By=2, Bx=3, H=40, W=50, fill=0, out=2 * p):
        return (frames, tc, block_shifts, By, Bx, H, W, fill, out, None)
    for kw in ({'frames': None}, {'block_shifts': None}, {'out': None}):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            warp(*warp_args(**kw))
    for kw in ({'tc': -1}, {'H': 0}, {'W': -1}, {'By': 0}, {'Bx': 0}):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative or zero'):
            warp(*warp_args(**kw))
    for kw, what in (({'By': 33}, 'limited to 32 x 32'), ({'Bx': 33}, 'limited to 32 x 32'), ({'H': 2 ** 15, 'W': 2 ** 15 + 1}, r'2\^30')):
        with pytest.raises(DcunetError, match=r'\(-3\).*' + what):
            warp(*warp_args(**kw))
    for kw in ({'H': 3, 'By': 4}, {'W': 2, 'Bx': 3}):
        with pytest.raises(DcunetError, match=r'\(-1\).*a block is empty'):
            warp(*warp_args(**kw))
    for fill in (65536, -32769):
        with pytest.raises(DcunetError, match=r'\(-1\).*fill = %d' % fill):
            warp(*warp_args(fill=fill))
    for kw in ({'frames': p + 1}, {'out': 2 * p + 1}, {'block_shifts': p + 2}):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            warp(*warp_args(**kw))
    for kw in ({'out': p}, {'tc': 2, 'out': p + 2 * 40 * 50}, {'tc': 2, 'frames': 2 * p, 'out': 2 * p - 2 * 40 * 50}):
        with pytest.raises(DcunetError, match=r'\(-1\).*out overlaps frames'):
            warp(*warp_args(**kw))
    assert warp(*warp_args(tc=0)) == 0


def test_geometry_and_field_under_the_host_sanitizers(tmp_path):
    """The block geometry and the field arithmetic of csrc/motion_math.h compiled into tests/native/motion_field_check.cpp with the
    address and undefined-behaviour sanitizers and run as a program of its own, against a brute-force restatement in 128-bit
    integers: int32 extremes, By = 1 and 32, axes up to 2^30."""
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
    exe = str(tmp_path / 'motion_field_check')
    src = os.path.join(ROOT, 'tests', 'native', 'motion_field_check.cpp')
    r = subprocess.run([cxx] + flags + [src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'motion_field_check: ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_frames_of_one_call_are_limited(dclib):
    """DC_FRAMES_PER_CALL_MAX: tc = 2^30 + 1 is refused with (-3) and the limit's message before any launch, tc = 2^30 is not."""
    import _wideindex
    _wideindex.check_frame_limit(dclib, 'test_motion_block_api')
