"""Temporal binning without a GPU: the public names and the ABI, argument validation in front of and inside the library, the
oracle of tests/_tbin_ref.py against its own naive and streaming restatements, the rounding of csrc/series_math.h as a stand-alone
program under the host sanitizers, the reach of split_rois on binned recordings, and the conditions the GPU scene relies on."""
import inspect
import itertools
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _pair_ref as pref
import _tbin_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT = dict(min_gap=0.1, min_area=8, iterations=16)


def test_public_names_and_abi():
    import deep_calcium_amd
    from deep_calcium_amd import _build, _gen_tape, _lib, footprints, roi_pairs, series, traces, dff
    assert deep_calcium_amd.TemporalBinner is series.TemporalBinner and 'TemporalBinner' in deep_calcium_amd.__all__
    assert _lib.header_abi_version() >= 121 and 'series.hip' in _build.SOURCES
    protos = _lib.parse_header()
    assert 'dc_series_bin_time' in protos and 'dc_series_bin_time' in set(n for n, _ in _gen_tape.prototypes())
    assert protos['dc_series_bin_time'][2] == ['frames', 'is_unsigned', 'tc', 'H', 'W', 'b', 'phase', 'carry', 'out', 'stream']
    header = open(_lib.HEADER).read()
    assert '#define DC_SERIES_MAX_BIN_FRAMES 64' in header and series.MAX_BIN_FRAMES == ref.MAX_BIN_FRAMES == 64
    assert 'dc_series_bin_round' in open(os.path.join(ROOT, 'deep_calcium_amd', 'csrc', 'series_math.h')).read()
    # bin_frames=None on the one-call functions that correlate, and on no other
    for fn in (series.summarize_series_device, footprints.roi_footprints_device, roi_pairs.roi_pair_corr_device, roi_pairs.split_rois_device):
        assert inspect.signature(fn).parameters['bin_frames'].default is None, fn.__name__
    for fn in (traces.extract_traces_device, dff.dff_traces_device):
        assert 'bin_frames' not in inspect.signature(fn).parameters, fn.__name__
    sig = inspect.signature(series.TemporalBinner.__init__).parameters
    assert list(sig)[1:] == ['shape', 'n_frames', 'dtype', 'bin_frames', 'shifts', 'fine_shifts', 'bidi', 'device', 'chunk_frames']
    assert sig['bin_frames'].default == 4


def test_module_imports_without_torch_or_the_library():
    code = ("import sys, deep_calcium_amd.series as m; from deep_calcium_amd import TemporalBinner; "
            "assert 'torch' not in sys.modules and 'deep_calcium_amd._lib' not in sys.modules; print(m.MAX_BIN_FRAMES)")
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == '64', out.stderr[-500:]


# ---- validation ----------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    from deep_calcium_amd import _lib, footprints, roi_pairs, series

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'lib', boom)
    B = series.TemporalBinner
    for args, kw, what in ((((5, 7), 8, np.float32), {}, 'int16 or uint16'),
                           (((5,), 8, np.int16), {}, 'shape'),
                           (((5, 7), 0, np.int16), {}, 'n_frames'),
                           (((5, 7), 8, np.int16), {'bin_frames': 0}, 'bin_frames'),
                           (((5, 7), 8, np.int16), {'bin_frames': -1}, 'bin_frames'),
                           (((5, 7), 100, np.int16), {'bin_frames': 65}, 'bin_frames'),
                           (((5, 7), 8, np.int16), {'bin_frames': 2.0}, 'bin_frames'),
                           (((5, 7), 8, np.int16), {'bin_frames': True}, 'bin_frames'),
                           (((5, 7), 8, np.int16), {'bin_frames': None}, 'bin_frames'),
                           (((5, 7), 3, np.int16), {'bin_frames': 4}, 'bin_frames'),
                           (((5, 7), 8, np.int16), {'chunk_frames': 0}, 'chunk_frames'),
                           (((5, 7), 8, np.int16), {'shifts': np.zeros((3, 2), int)}, 'shifts'),
                           (((5, 7), 8, np.int16), {'bidi': 7}, 'bidi'),
                           (((5, 7), 8, np.int16), {'shifts': np.zeros((8, 2), int), 'fine_shifts': np.zeros((8, 2), int)}, 'not both')):
        with pytest.raises(ValueError, match=what):
            B(*args, **kw)
    ok = [np.array([[1, 2], [3, 4]])]
    missing = '/nonexistent/dataset.npz'
    for bad in (0, 65, 2.0, True, 'x'):
        for call in (lambda: series.summarize_series_device(missing, kind='corr', bin_frames=bad),
                     lambda: footprints.roi_footprints_device(missing, ok, bin_frames=bad),
                     lambda: roi_pairs.roi_pair_corr_device(missing, ok, bin_frames=bad),
                     lambda: roi_pairs.split_rois_device(missing, ok, bin_frames=bad)):
            with pytest.raises(ValueError, match='bin_frames'):
                call()


def test_c_abi_argument_validation_returns_codes(dclib):
    """Refused before any launch (there is no GPU here): the pointers are never followed."""
    from deep_calcium_amd._lib import DcunetError
    p = 1 << 20                               # any aligned non-null value; the buffers below lie far apart

    def F(frames=p, uns=0, tc=4, H=5, W=7, b=4, phase=0, carry=2 * p, out=3 * p):
        return dclib.dc_series_bin_time(frames, uns, tc, H, W, b, phase, carry, out, None)
    for kw in (dict(b=0), dict(b=-3), dict(phase=-1), dict(phase=4), dict(b=1, phase=1), dict(b=64, phase=64)):
        with pytest.raises(DcunetError, match=r'\(-1\)'):
            F(**kw)
    for kw in (dict(b=65), dict(b=65, phase=64), dict(b=2 ** 20), dict(H=2 ** 15, W=2 ** 15 + 1)):
        with pytest.raises(DcunetError, match=r'\(-3\)'):
            F(**kw)
    for kw in (dict(tc=-1), dict(H=0), dict(W=-2)):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative or zero'):
            F(**kw)
    # a null pointer that would be followed: frames always, out when a bin closes, carry when a bin is or stays open
    for kw in (dict(frames=None), dict(out=None), dict(carry=None, phase=1), dict(carry=None, tc=5), dict(carry=None, tc=2, out=None)):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            F(**kw)
    for kw in (dict(frames=p + 1), dict(out=3 * p + 1), dict(carry=2 * p + 2)):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            F(**kw)
    n = 2 * 5 * 7                             # bytes of one frame
    for kw in (dict(out=p), dict(out=p + 4 * n - 2), dict(out=p - n + 2)):
        with pytest.raises(DcunetError, match=r'\(-1\).*out overlaps frames'):
            F(**kw)
    for kw in (dict(out=2 * p, phase=1), dict(out=2 * p + 2 * n - 2, tc=5), dict(out=2 * p - n + 2, tc=5)):
        with pytest.raises(DcunetError, match=r'\(-1\).*out overlaps carry'):
            F(**kw)
    with pytest.raises(DcunetError, match=r'\(-1\).*carry overlaps frames'):
        F(carry=p + 4 * n - 4, tc=5)
    # tc == 0 launches nothing, whatever the pointers; checked all the same
    assert F(tc=0) == 0 and F(tc=0, frames=None, carry=None, out=None) == 0 and F(tc=0, b=64, phase=63) == 0
    with pytest.raises(DcunetError, match=r'\(-3\)'):
        F(tc=0, b=65)


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def _rand(rs, shape, dtype):
    info = np.iinfo(dtype)
    return rs.randint(info.min, info.max + 1, size=shape).astype(dtype)


def test_oracle_properties():
    rs = np.random.RandomState(3)
    for dtype in (np.int16, np.uint16):
        info = np.iinfo(dtype)
        f = _rand(rs, (24, 3, 5), dtype)
        f[0, 0, 0], f[1, 0, 0], f[5, 1, 1], f[7, 1, 1] = info.min, info.max, info.max, info.min
        assert np.array_equal(ref.bin_time(f, 1), f) and ref.bin_time(f, 1).dtype == dtype               # b = 1 is the identity
        for b in (2, 3, 5, 7, 24):
            got = ref.bin_time(f, b)
            n = 24 // b
            assert got.shape == (n, 3, 5) and got.dtype == dtype
            groups = f[:n * b].reshape(n, b, 3, 5).astype(np.int64)
            assert (got >= groups.min(1)).all() and (got <= groups.max(1)).all()                         # between the bin's min and max
            exact = groups.sum(1) / float(b)
            assert (np.abs(got - exact) <= 0.5).all() and (got[np.abs(got - exact) == 0.5] > exact[np.abs(got - exact) == 0.5]).all()
        small = f[:12, :2, :3]
        for b in (1, 2, 3, 5):
            assert np.array_equal(ref.bin_time(small, b), ref.bin_time_naive(small, b))
    assert ref.bin_time(np.array([-1, -2], np.int16).reshape(2, 1, 1), 2).tolist() == [[[-1]]]           # -1.5 rounds half UP
    assert ref.bin_time(np.array([-2, -3], np.int16).reshape(2, 1, 1), 2).tolist() == [[[-2]]]
    assert ref.bin_time(np.array([1, 2], np.int16).reshape(2, 1, 1), 2).tolist() == [[[2]]]
    assert ref.bin_time(np.full((64, 1, 1), -32768, np.int16), 64).tolist() == [[[-32768]]]
    assert ref.bin_time(np.full((64, 1, 1), 32767, np.int16), 64).tolist() == [[[32767]]]
    assert ref.bin_time(np.full((64, 1, 1), 65535, np.uint16), 64).tolist() == [[[65535]]]
    assert ref.bin_time(np.zeros((3, 2, 2), np.int16), 4).shape == (0, 2, 2)


def test_streaming_restatement_equals_the_oracle_for_every_split():
    rs = np.random.RandomState(4)
    T, b = 11, 3
    for dtype in (np.int16, np.uint16):
        f = _rand(rs, (T, 2, 3), dtype)
        want = ref.bin_time(f, b)
        assert want.shape[0] == 3
        count = 0
        for k in range(T):
            for cuts in itertools.combinations(range(1, T), k):
                assert np.array_equal(ref.stream_all(f, b, cuts), want), cuts
                count += 1
        assert count == 2 ** (T - 1)
    # one call by the words of the contract
    out, carry, phase = ref.stream(f[:2], 3, 0, None)
    assert out.shape[0] == 0 and phase == 2 and np.array_equal(carry, f[:2].astype(np.int64).sum(0))
    out, carry, phase = ref.stream(f[2:3], 3, 2, carry)
    assert out.shape[0] == 1 and phase == 0 and carry is None and np.array_equal(out, want[:1])


# ---- the scalar arithmetic of the kernel -------------------------------------------------------------------------------------
def test_bin_rounding_under_the_host_sanitizers(tmp_path):
    """The rounding of csrc/series_math.h compiled into tests/native/series_bin_check.cpp with the address and
    undefined-behaviour sanitizers and run as a program of its own: every b in [1, 64] against 64-bit floor division at the
    extremes of both types, around every half and around zero."""
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
    exe = str(tmp_path / 'series_bin_check')
    src = os.path.join(ROOT, 'tests', 'native', 'series_bin_check.cpp')
    r = subprocess.run([cxx] + flags + [src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'series_bin_check: ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


# ---- the reach of the split rule on binned recordings ------------------------------------------------------------------------
def _wrong(new, left, right):
    """Pixels of the two parts that are not where they were planted, plus pixels of the region in neither part."""
    sets = [set(map(tuple, p.tolist())) for p in new]
    want = [set(map(tuple, left.tolist())), set(map(tuple, right.tolist()))]
    return len(sets[0] - want[0]) + len(sets[1] - want[1]) + len((want[0] | want[1]) - (sets[0] | sets[1]))


def _split_binned(frames, region, b):
    from deep_calcium_amd import split_rois
    binned = ref.bin_time(frames, b) if b > 1 else frames
    return split_rois([region], [pref.corrcoef(binned, region)], frames.shape[1:], **SPLIT)


REACH = ((60.0, 30.0), (40.0, 40.0), (30.0, 60.0), (20.0, 60.0))
BINS = (1, 2, 4, 8, 16)


def test_the_reach_of_the_split_rule_on_binned_recordings():
    """The T = 1024 rows of the README's table, np.corrcoef of the oracle's binned frames standing in for the device, 40 seeds per
    cell: `split / split with any pixel misassigned or dropped` of the two-cell scene, and how many controls split."""
    table, controls = {}, {}
    for amp, sigma in REACH:
        two = [pref.scene('two', seed, amplitude=amp, sigma=sigma, T=1024) for seed in range(40)]
        for b in BINS:
            split = wrong = 0
            for frames, region, left, right, _ in two:
                new, origin, gaps = _split_binned(frames, region, b)
                if len(new) == 2:
                    split += 1
                    wrong += _wrong(new, left, right) > 0
            table[amp, sigma, b] = (split, wrong)
        if (amp, sigma) in ((40.0, 40.0), (30.0, 60.0)):
            for kind in ('same', 'gauss', 'static'):
                for seed in range(40):
                    frames, region = pref.scene(kind, seed, amplitude=amp, sigma=sigma, T=1024)[:2]
                    for b in (4, 8):
                        controls[amp, sigma, b] = controls.get((amp, sigma, b), 0) + (len(_split_binned(frames, region, b)[0]) == 2)
    print('\nT = 1024, scenes split of 40 / with a wrong pixel')
    print('amplitude / sigma  ' + ''.join('b=%-7d' % b for b in BINS))
    for amp, sigma in REACH:
        print('%9.0f / %-6.0f ' % (amp, sigma) + ''.join('%2d/%-6d' % table[amp, sigma, b] for b in BINS))
    print('controls split: %r' % (sorted(controls.items()),))
    assert table[40.0, 40.0, 4] == (40, 0)                                              # all split exactly
    assert controls[40.0, 40.0, 4] == 0 and controls[40.0, 40.0, 8] == 0                # and no control
    assert table[40.0, 40.0, 1][0] < 40                                                 # which the single frames do not reach
    split, wrong = table[30.0, 60.0, 8]
    assert split >= 35 and wrong <= 6
    assert table[30.0, 60.0, 1] == (0, 0) and controls[30.0, 60.0, 8] == 0


def test_the_gpu_scene_meets_its_conditions_on_the_reference():
    """What tests/test_tbin_gpu.py relies on: on the float64 oracle the seed-11 scene at 40 / 40, T = 1024, is NOT split frame by
    frame (gap at least 0.015 below min_gap) and IS split into exactly the planted halves at b = 4 (gap at least 0.1 above
    min_gap); the three controls of the seed stay whole at b = 4 with gaps of at most 0.02.  Margins far beyond a float32 ulp of
    the matrix."""
    frames, region, left, right, _ = pref.scene('two', 11, amplitude=40.0, sigma=40.0, T=1024)
    assert frames.shape == (1024, 10, 16) and frames.dtype == np.int16
    new, origin, gaps = _split_binned(frames, region, 1)
    print('unbinned gap %.3f' % gaps[0])
    assert len(new) == 1 and np.array_equal(new[0], region) and gaps[0] <= SPLIT['min_gap'] - 0.015
    new, origin, gaps = _split_binned(frames, region, 4)
    print('b = 4 gap %.3f' % gaps[0])
    assert origin == [0, 0] and np.array_equal(new[0], left) and np.array_equal(new[1], right) and gaps[0] >= SPLIT['min_gap'] + 0.1
    for kind in ('same', 'gauss', 'static'):
        f, r = pref.scene(kind, 11, amplitude=40.0, sigma=40.0, T=1024)[:2]
        new, origin, gaps = _split_binned(f, r, 4)
        print('%s at b = 4: gap %.3f' % (kind, gaps[0]))
        assert len(new) == 1 and not gaps[0] > 0.02, (kind, gaps[0])


def test_frames_of_one_call_are_limited(dclib):
    """DC_FRAMES_PER_CALL_MAX: tc = 2^30 + 1 is refused with (-3) and the limit's message before any launch, tc = 2^30 is not."""
    import _wideindex
    _wideindex.check_frame_limit(dclib, 'test_tbin_api')
