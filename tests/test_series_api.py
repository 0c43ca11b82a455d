"""Series summaries without a GPU: the public names, the ABI revision, argument validation in front of the library, and the
exact scalar helpers of the kernels (csrc/series_math.h) as a stand-alone program under the host sanitizers."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_public_names_and_abi_revision():
    import deep_calcium_amd
    from deep_calcium_amd import _gen_tape, _lib, series
    assert deep_calcium_amd.SeriesSummarizer is series.SeriesSummarizer
    assert deep_calcium_amd.summarize_series_device is series.summarize_series_device
    assert {'SeriesSummarizer', 'summarize_series_device'} <= set(deep_calcium_amd.__all__)
    assert _lib.header_abi_version() >= 108
    protos = _lib.parse_header()
    tapeable = set(n for n, _ in _gen_tape.prototypes())
    for name in ('dc_series_accumulate', 'dc_series_accumulate_xy', 'dc_series_finalize', 'dc_image_standardize'):
        assert name in protos and name in tapeable, name
    assert 'dc_series_standardize_ws_floats' in protos and 'dc_series_standardize_ws_floats' not in tapeable
    header = open(_lib.HEADER).read()
    assert 'datasets/nf.py:121-130' in header and 'unet_2d_summary.py:227-241' in header
    assert 'DC_SERIES_MAX_FRAMES 2147483647' in header and series.MAX_FRAMES == 2147483647


def test_series_module_imports_without_torch_or_the_library():
    code = ("import sys, deep_calcium_amd.series as s; "
            "assert 'torch' not in sys.modules and 'deep_calcium_amd._lib' not in sys.modules; print(','.join(s.KINDS))")
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == 'mean16,max16,mean,max,std,corr', out.stderr[-500:]


def test_argument_validation_fires_before_the_library_is_touched(monkeypatch):
    from deep_calcium_amd import _lib, series

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'lib', boom)
    S = series.SeriesSummarizer
    for args, kw, what in ((((5, 7), 4, np.float32), {}, 'int16 or uint16'),
                           (((5, 7), 4, 'no-such-type'), {}, 'int16 or uint16'),
                           (((5,), 4, np.int16), {}, 'shape'),
                           (((5, 0), 4, np.int16), {}, 'shape'),
                           ((7, 4, np.int16), {}, 'shape'),
                           (((5, 7), 0, np.int16), {}, 'n_frames'),
                           (((5, 7), 2 ** 31, np.int16), {}, 'n_frames'),
                           (((5, 7), 4, np.int16), {'kinds': ('mean', 'median')}, 'not one of'),
                           (((5, 7), 4, np.int16), {'kinds': ()}, 'empty'),
                           (((5, 7), 4, np.int16), {'chunk_frames': 0}, 'chunk_frames')):
        with pytest.raises(ValueError, match=what):
            S(*args, **kw)
    with pytest.raises(ValueError, match='not one of'):
        series.summarize_series_device('/nonexistent/dataset.npz', kind='median')


def test_memory_mapped_npz_member_is_the_stored_array(tmp_path):
    from deep_calcium_amd import hdf5_min, series
    raw = np.arange(3 * 4 * 5, dtype=np.int16).reshape(3, 4, 5) - 17
    p = str(tmp_path / 'a.npz')
    np.savez(p, name=np.array('x'), series_raw=raw, series_mean=np.zeros((4, 5), np.float16))
    arr, close = series._open_series(p, 'series/raw')
    assert isinstance(arr, np.memmap) and arr.dtype == np.int16 and np.array_equal(arr, raw)
    close()
    p = str(tmp_path / 'c.npz')
    np.savez_compressed(p, series_raw=raw)
    arr, close = series._open_series(p, 'series/raw')
    assert np.array_equal(arr, raw)
    close()
    with pytest.raises(ValueError, match='no member'):
        series._open_series(p, 'series/other')
    # the built-in HDF5 reader hands out the dataset in place
    w = hdf5_min.Writer()
    w.create_dataset('series/raw', data=raw)
    p = str(tmp_path / 'd.hdf5')
    w.save(p)
    f = hdf5_min.File(p)
    v = f['series/raw'].view()
    assert v.dtype == np.int16 and not v.flags.writeable and np.array_equal(v, raw)
    del v
    f.close()
    # through _open_series (no h5py here: the built-in reader); close() tolerates a slice that is still alive, as when a
    # traceback holds one, so that it cannot mask the error that is propagating
    arr, close = series._open_series(p, 'series/raw')
    assert np.array_equal(arr, raw)
    try:
        import h5py  # noqa: F401
    except ImportError:
        assert not arr.flags.owndata
    part = arr[1:2]
    close()
    del arr, part
    with pytest.raises(ValueError, match='no dataset'):
        series._open_series(p, 'series/other')


def test_scalar_helpers_under_the_host_sanitizers(tmp_path):
    """csrc/series_math.h (double -> half with one rounding, 128-bit numerators) compiled into tests/native/series_math_check.cpp
    with the address and undefined-behaviour sanitizers and run as a program of its own."""
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
    exe = str(tmp_path / 'series_math_check')
    src = os.path.join(ROOT, 'tests', 'native', 'series_math_check.cpp')
    r = subprocess.run([cxx] + flags + [src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'series_math_check: ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_frames_of_one_call_are_limited(dclib):
    """DC_FRAMES_PER_CALL_MAX: tc = 2^30 + 1 is refused with (-3) and the limit's message before any launch, tc = 2^30 is not."""
    import _wideindex
    _wideindex.check_frame_limit(dclib, 'test_series_api')
