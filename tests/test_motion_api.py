"""Motion correction without a GPU: the public names and the ABI, argument validation in front of and inside the library, the
valid rectangle, and the tie rule of csrc/motion_math.h as a stand-alone program under the host sanitizers."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_public_names_and_abi():
    import deep_calcium_amd
    from deep_calcium_amd import _build, _gen_tape, _lib, motion
    for name in ('MotionCorrector', 'make_template', 'estimate_shifts_device', 'valid_rectangle'):
        assert getattr(deep_calcium_amd, name) is getattr(motion, name) and name in deep_calcium_amd.__all__
    assert _lib.header_abi_version() >= 112 and 'motion.hip' in _build.SOURCES
    protos = _lib.parse_header()
    tapeable = set(n for n, _ in _gen_tape.prototypes())
    for name in ('dc_motion_ssd', 'dc_motion_pick', 'dc_motion_apply'):
        assert name in protos and name in tapeable, name
        assert protos[name][2][-1] == 'stream'
    header = open(_lib.HEADER).read()
    assert 'DC_MOTION_MAX_SHIFT 16' in header and motion.MAX_SHIFT == 16
    for text in (header, motion.__doc__, open(os.path.join(ROOT, 'README.md')).read()):
        assert '(dy, dx) = (-a, -b)' in text             # the sign convention is stated where a user looks


def test_motion_module_imports_without_torch_or_the_library():
    code = ("import sys, deep_calcium_amd.motion as m; "
            "assert 'torch' not in sys.modules and 'deep_calcium_amd._lib' not in sys.modules; print(m.MAX_SHIFT)")
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == '16', out.stderr[-500:]


def test_valid_rectangle():
    from deep_calcium_amd import valid_rectangle
    assert valid_rectangle(np.zeros((3, 2), np.int32), (10, 12)) == ((0, 10), (0, 12))
    assert valid_rectangle([[2, -3], [-1, 4], [0, 0]], (10, 12)) == ((1, 8), (3, 8))
    assert valid_rectangle([[-5, -5]], (10, 12)) == ((5, 10), (5, 12))
    assert valid_rectangle(np.zeros((0, 2), np.int32), (10, 12)) == ((0, 10), (0, 12))


def _boom(*a, **k):
    raise AssertionError('the library was touched')


def test_corrector_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    from deep_calcium_amd import _lib, motion
    monkeypatch.setattr(_lib, 'lib', _boom)
    t16, tu16 = np.zeros((40, 50), np.int16), np.zeros((40, 50), np.uint16)
    M = motion.MotionCorrector
    for args, kw, what in ((((40, 50), 4, np.float32, t16), {}, 'int16 or uint16'),
                           (((40,), 4, np.int16, t16), {}, 'shape'),
                           (((40, 50), 0, np.int16, t16), {}, 'n_frames'),
                           (((40, 50), 4, np.int16, tu16), {}, 'template is uint16'),
                           (((40, 50), 4, np.uint16, t16), {}, 'template is int16'),
                           (((40, 50), 4, np.int16, t16[:, :49]), {}, 'template is'),
                           (((40, 50), 4, np.int16, t16.tolist()), {}, 'template must be a numpy array'),
                           (((40, 50), 4, np.int16, t16), {'max_shift': 17}, r'max_shift must be in \[0, 16\]'),
                           (((40, 50), 4, np.int16, t16), {'max_shift': -1}, r'max_shift must be in \[0, 16\]'),
                           (((40, 50), 4, np.int16, t16), {'max_shift': 2.5}, 'max_shift must be an integer'),
                           (((32, 50), 4, np.int16, t16[:32]), {'max_shift': 16}, r'max_shift = 16 leaves no interior.*H > 2 \* max_shift'),
                           (((40, 16), 4, np.int16, t16[:, :16]), {'max_shift': 8}, 'max_shift = 8 leaves no interior'),
                           (((40, 50), 4, np.int16, t16), {'fill': 70000}, 'fill'),
                           (((40, 50), 4, np.int16, t16), {'fill': 1.5}, 'fill'),
                           (((40, 50), 4, np.int16, t16), {'chunk_frames': 0}, 'chunk_frames')):
        with pytest.raises(ValueError, match=what):
            M(*args, **kw)
    frames = np.zeros((3, 40, 50), np.int16)
    for args, kw, what in (((frames.astype(np.float32),), {}, 'int16 or uint16'),
                           ((frames[0],), {}, r'\(N, H, W\)'),
                           ((frames,), {'max_shift': 20}, 'max_shift'),
                           ((frames[:, :, :10],), {'max_shift': 5}, 'leaves no interior'),
                           ((frames,), {'iterations': -1}, 'iterations')):
        with pytest.raises(ValueError, match=what):
            motion.make_template(*args, **kw)
    for kw, what in (({'max_shift': 17}, 'max_shift'), ({'template_frames': 0}, 'template_frames')):
        with pytest.raises(ValueError, match=what):
            motion.estimate_shifts_device('/nonexistent/dataset.npz', **kw)


def test_shifts_keyword_is_checked_before_the_library_is_touched(monkeypatch):
    from deep_calcium_amd import _lib, series, traces
    monkeypatch.setattr(_lib, 'lib', _boom)
    ok = [np.array([[1, 2], [3, 4]])]
    for bad in (np.zeros((5, 2), np.int32), np.zeros((4, 3), np.int32), np.zeros(8, np.int32), np.zeros((4, 2), np.float32),
                [[0, 0]] * 3, np.array([[0, 2 ** 31]] * 4)):
        with pytest.raises(ValueError, match='shifts must'):
            series.SeriesSummarizer((5, 7), 4, np.int16, shifts=bad)
        with pytest.raises(ValueError, match='shifts must'):
            traces.RoiTraceExtractor((5, 7), 4, np.int16, ok, shifts=bad)
    assert series._check_shifts(None, 4) is None
    good = series._check_shifts([[1, -2]] * 4, 4)
    assert good.dtype == np.int32 and good.shape == (4, 2) and good.flags.c_contiguous


def test_feeding_more_frames_than_declared_is_refused():
    """feed()'s checks run before anything is launched: a corrector that never reached the GPU is enough to exercise them."""
    from deep_calcium_amd import motion
    mc = motion.MotionCorrector.__new__(motion.MotionCorrector)
    mc.shape, mc.n_frames, mc.dtype, mc.fed, mc.chunk_frames = (40, 50), 4, np.dtype(np.int16), 3, 4
    mc._torch = None
    with pytest.raises(ValueError, match='2 frames after 3 fed: the recording was declared to have 4'):
        mc.feed(np.zeros((2, 40, 50), np.int16))
    with pytest.raises(ValueError, match='frames are uint16'):
        mc.feed(np.zeros((1, 40, 50), np.uint16))
    with pytest.raises(ValueError, match=r'frames must be \(t, 40, 50\)'):
        mc.feed(np.zeros((1, 40, 51), np.int16))
    with pytest.raises(ValueError, match='frames must be a numpy array'):
        mc.feed([[0]])


def test_c_abi_argument_validation_returns_codes(dclib):
    """Refused before any launch (there is no GPU here): the pointers are never followed."""
    from deep_calcium_amd._lib import DcunetError
    p = 4096                                  # any aligned non-null value
    ssd, pick, app = dclib.dc_motion_ssd, dclib.dc_motion_pick, dclib.dc_motion_apply
    for args in ((None, 0, 1, p, 40, 50, 8, p, None), (p, 0, 1, None, 40, 50, 8, p, None), (p, 0, 1, p, 40, 50, 8, None, None)):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            ssd(*args)
    for H, W, S in ((16, 50, 8), (40, 16, 8), (1, 50, 1), (32, 33, 16)):
        with pytest.raises(DcunetError, match=r'\(-1\).*no interior'):
            ssd(p, 0, 1, p, H, W, S, p, None)
    with pytest.raises(DcunetError, match=r'\(-3\).*limited to 16'):
        ssd(p, 0, 1, p, 400, 500, 17, p, None)
    with pytest.raises(DcunetError, match=r'\(-3\).*2\^30'):
        ssd(p, 0, 1, p, 2 ** 15, 2 ** 15 + 1, 8, p, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
        ssd(p, 0, -1, p, 40, 50, 8, p, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
        ssd(p, 0, 1, p, 40, 50, -1, p, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
        ssd(p + 1, 0, 1, p, 40, 50, 8, p, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
        ssd(p, 0, 1, p, 40, 50, 8, p + 4, None)
    assert ssd(p, 0, 0, p, 40, 50, 8, p, None) == 0          # no frames: nothing launched
    with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
        pick(None, 1, 8, p, None, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
        pick(p, 1, 8, None, None, None)
    with pytest.raises(DcunetError, match=r'\(-3\).*limited to 16'):
        pick(p, 1, 17, p, None, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
        pick(p, 1, 8, p + 2, None, None)
    assert pick(p, 0, 8, p, None, None) == 0
    for args in ((None, 1, p, 40, 50, 0, 2 * p, None), (p, 1, None, 40, 50, 0, 2 * p, None), (p, 1, p, 40, 50, 0, None, None)):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            app(*args)
    with pytest.raises(DcunetError, match=r'\(-1\).*fill = 65536'):
        app(p, 1, p, 40, 50, 65536, 2 * p, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*out overlaps frames'):
        app(p, 1, p, 40, 50, 0, p, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*out overlaps frames'):
        app(p, 2, p, 40, 50, 0, p + 2 * 40 * 50, None)
    with pytest.raises(DcunetError, match=r'\(-3\).*2\^30'):
        app(p, 1, p, 2 ** 15, 2 ** 15 + 1, 0, 2 * p, None)
    assert app(p, 0, p, 40, 50, 0, 2 * p, None) == 0


def test_tie_rule_under_the_host_sanitizers(tmp_path):
    """dc_motion_before / dc_motion_cand / dc_motion_pick_serial of csrc/motion_math.h compiled into
    tests/native/motion_math_check.cpp with the address and undefined-behaviour sanitizers and run as a program of its own."""
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
    exe = str(tmp_path / 'motion_math_check')
    src = os.path.join(ROOT, 'tests', 'native', 'motion_math_check.cpp')
    r = subprocess.run([cxx] + flags + [src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'motion_math_check: ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_frames_of_one_call_are_limited(dclib):
    """DC_FRAMES_PER_CALL_MAX: tc = 2^30 + 1 is refused with (-3) and the limit's message before any launch, tc = 2^30 is not."""
    import _wideindex
    _wideindex.check_frame_limit(dclib, 'test_motion_api')
