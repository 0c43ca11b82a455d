"""ROI traces without a GPU: the public names and the ABI, rois_to_csr (deep_calcium_amd/traces.py), argument validation in front
of and inside the library, the traces dataset file, and the 128-bit helpers the kernels add to csrc/series_math.h as a
stand-alone program under the host sanitizers."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_public_names_and_abi():
    import deep_calcium_amd
    from deep_calcium_amd import _gen_tape, _lib, traces
    for name in ('RoiTraceExtractor', 'rois_to_csr', 'extract_traces_device', 'write_traces_dataset'):
        assert getattr(deep_calcium_amd, name) is getattr(traces, name) and name in deep_calcium_amd.__all__
    assert _lib.header_abi_version() >= 109
    protos = _lib.parse_header()
    tapeable = set(n for n, _ in _gen_tape.prototypes())
    for name in ('dc_roi_trace_accumulate', 'dc_roi_trace_finalize'):
        assert name in protos and name in tapeable, name
    header = open(_lib.HEADER).read()
    assert 'unet_1d_segmentation.py:182-187' in header and 'unet_1d_segmentation.py:158-167' in header
    assert 'DC_ROI_TRACE_MAX_VOLUME 70368744177664' in header and traces.MAX_VOLUME == 70368744177664 == 2 ** 46
    assert traces.SEGMENT_PIXELS * 65535 < 2 ** 31          # a row's sum over one frame fits int32


def test_traces_module_imports_without_torch_or_the_library():
    code = ("import sys, deep_calcium_amd.traces as t; "
            "assert 'torch' not in sys.modules and 'deep_calcium_amd._lib' not in sys.modules; print(','.join(t.KINDS))")
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == 'sum,mean,zscore', out.stderr[-500:]


# ---- rois_to_csr ---------------------------------------------------------------------------------------------------------
def _rows(csr):
    areas, off, pix, roi = csr
    return [(int(roi[s]), pix[off[s]:off[s + 1]]) for s in range(len(roi))]


def _check_invariants(csr, want_pixels):
    """want_pixels: per ROI the sorted unique flat indices."""
    from deep_calcium_amd.traces import SEGMENT_PIXELS
    areas, off, pix, roi = csr
    for a in csr:
        assert a.dtype == np.int32 and a.ndim == 1
    assert len(off) == len(roi) + 1 and off[0] == 0 and off[-1] == len(pix) and (np.diff(off) >= 1).all()
    assert (np.diff(off) <= SEGMENT_PIXELS).all()
    assert (np.diff(roi) >= 0).all() and sorted(set(roi.tolist())) == list(range(len(want_pixels)))
    assert areas.tolist() == [len(p) for p in want_pixels]
    for r, want in enumerate(want_pixels):
        parts = [p for rr, p in _rows(csr) if rr == r]
        assert len(parts) == -(-len(want) // SEGMENT_PIXELS)
        assert all(len(p) == SEGMENT_PIXELS for p in parts[:-1])
        assert np.array_equal(np.concatenate(parts), want), r


def test_the_four_input_forms_describe_the_same_rois():
    from deep_calcium_amd.nf_metrics import mask_to_regions
    from deep_calcium_amd.traces import SEGMENT_PIXELS, rois_to_csr
    H, W = 40, 70
    mask = np.zeros((H, W), np.uint8)
    mask[2:5, 3:9] = 1                        # 18 pixels
    mask[10:39, 20:69] = 1                    # 29 x 49 = 1421 pixels: three segments
    mask[7, 0] = 1                            # a single pixel
    regions = mask_to_regions(mask)
    assert [len(r) for r in regions] == [18, 1, 1421] and 1421 > 2 * SEGMENT_PIXELS
    stack = np.zeros((3, H, W), np.int8)
    for i, r in enumerate(regions):
        stack[i, r[:, 0], r[:, 1]] = 1
    rs = np.random.RandomState(0)
    shuffled = [np.concatenate([r, r[:3]])[rs.permutation(len(r) + len(r[:3]))] for r in regions]      # any order, up to three pixels twice
    dicts = [{'coordinates': [[int(y), int(x)] for y, x in r]} for r in regions]
    want = [np.sort(r[:, 0] * W + r[:, 1]) for r in regions]
    ref = rois_to_csr(mask, (H, W))
    _check_invariants(ref, want)
    for form in (stack, shuffled, dicts, tuple(regions)):
        got = rois_to_csr(form, (H, W))
        for a, b in zip(ref, got):
            assert a.dtype == b.dtype and np.array_equal(a, b)
    # overlapping and identical ROIs stay separate ROIs
    csr = rois_to_csr([regions[0], regions[0], regions[0][:5]], (H, W))
    _check_invariants(csr, [want[0], want[0], np.sort(want[0][:5])])


def test_region_order_is_mask_to_regions_order(golden_dir):
    from deep_calcium_amd.nf_metrics import mask_to_regions
    from deep_calcium_amd.traces import rois_to_csr
    g = np.load(os.path.join(golden_dir, 'nf.npz'))
    seen = 0
    for i in range(4):
        m = g['mask_%d' % i]
        regions = mask_to_regions(m)
        if not regions:
            with pytest.raises(ValueError, match='no ROIs'):
                rois_to_csr(m, m.shape)
            continue
        seen += 1
        _check_invariants(rois_to_csr(m, m.shape), [np.sort(r[:, 0] * m.shape[1] + r[:, 1]) for r in regions])
    assert seen >= 2
    # two regions that touch only diagonally are ONE region (8-connected); the one that starts later in raster order comes later
    m = np.array([[0, 0, 0, 1, 1],
                  [1, 1, 0, 0, 0],
                  [0, 0, 1, 0, 0],
                  [0, 0, 0, 0, 1]], np.uint8)
    areas, off, pix, roi = rois_to_csr(m, m.shape)
    assert areas.tolist() == [2, 3, 1] and pix.tolist() == [3, 4, 5, 6, 12, 19] and roi.tolist() == [0, 1, 2]


def test_rois_to_csr_refuses_what_it_cannot_represent():
    from deep_calcium_amd.traces import rois_to_csr
    ok = np.array([[1, 2], [3, 4]])
    for rois, shape, what in (([ok, np.zeros((0, 2), int)], (5, 7), 'ROI 1 is empty'),
                              (np.zeros((2, 5, 7), np.int8), (5, 7), 'ROI 0 is empty'),
                              ([{'coordinates': []}], (5, 7), 'empty'),
                              ([np.array([[1, 7]])], (5, 7), 'outside'),
                              ([np.array([[5, 0]])], (5, 7), 'outside'),
                              ([np.array([[-1, 0]])], (5, 7), 'outside'),
                              ([], (5, 7), 'no ROIs'),
                              (np.zeros((5, 7), np.uint8), (5, 7), 'no ROIs'),
                              (np.zeros((0, 5, 7), np.uint8), (5, 7), 'no ROIs'),
                              (np.ones((7, 5), np.uint8), (5, 7), 'the frames are'),
                              (np.ones((2, 7, 5), np.uint8), (5, 7), 'the frames are'),
                              ([np.array([1, 2, 3])], (5, 7), r'\(k,2\)'),
                              ([np.array([[1.5, 2.0]])], (5, 7), r'\(k,2\)'),
                              ('mask', (5, 7), 'rois must be'),
                              ([ok], (5,), 'shape'),
                              ([ok], (0, 7), 'shape')):
        with pytest.raises(ValueError, match=what):
            rois_to_csr(rois, shape)


# ---- validation ----------------------------------------------------------------------------------------------------------
def test_extractor_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    from deep_calcium_amd import _lib, traces

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'lib', boom)
    ok = [np.array([[1, 2], [3, 4]])]
    E = traces.RoiTraceExtractor
    for args, kw, what in ((((5, 7), 4, np.float32, ok), {}, 'int16 or uint16'),
                           (((5,), 4, np.int16, ok), {}, 'shape'),
                           (((5, 0), 4, np.int16, ok), {}, 'shape'),
                           (((5, 7), 0, np.int16, ok), {}, 'n_frames'),
                           (((5, 7), 2 ** 46 // 35 + 1, np.int16, ok), {}, r'2\*\*46'),
                           (((5, 7), 4, np.int16, []), {}, 'no ROIs'),
                           (((5, 7), 4, np.int16, [np.array([[5, 7]])]), {}, 'outside'),
                           (((5, 7), 4, np.int16, np.ones((7, 5), np.uint8)), {}, 'the frames are'),
                           (((5, 7), 4, np.int16, ok), {'chunk_frames': 0}, 'chunk_frames')):
        with pytest.raises(ValueError, match=what):
            E(*args, **kw)
    with pytest.raises(ValueError, match='not one of'):
        traces.extract_traces_device('/nonexistent/dataset.npz', ok, kind='median')


def test_c_abi_argument_validation_returns_codes(dclib):
    """Refused before any launch (there is no GPU here): the pointers are never followed."""
    from deep_calcium_amd._lib import DcunetError
    p = 4096                                  # any aligned non-null value
    acc, fin = dclib.dc_roi_trace_accumulate, dclib.dc_roi_trace_finalize
    for args in ((None, 0, 1, 0, p, p, None, 1, 1, p, 1, 5, 7, None), (p, 0, 1, 0, None, p, None, 1, 1, p, 1, 5, 7, None),
                 (p, 0, 1, 0, p, None, None, 1, 1, p, 1, 5, 7, None), (p, 0, 1, 0, p, p, None, 1, 1, None, 1, 5, 7, None)):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            acc(*args)
    with pytest.raises(DcunetError, match=r'\(-1\).*ld = 7 is below t0 \+ tc = 8'):
        acc(p, 0, 3, 5, p, p, None, 1, 1, p, 7, 5, 7, None)
    for S, R, tc, t0 in ((-1, 1, 1, 0), (1, -1, 1, 0), (1, 1, -1, 0), (1, 1, 1, -1)):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
            acc(p, 0, tc, t0, p, p, p, S, R, p, 8, 5, 7, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*S = 2 and R = 3'):
        acc(p, 0, 1, 0, p, p, None, 2, 3, p, 8, 5, 7, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*out of range'):
        acc(p, 0, 1, 0, p, p, None, 1, 1, p, 8, 2 ** 15, 2 ** 15 + 1, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
        acc(p + 1, 0, 1, 0, p, p, None, 1, 1, p, 8, 5, 7, None)
    # the limit T * H * W <= 2^46: the last frame that fits is accepted by the check (and R == 0 launches nothing)
    T = 2 ** 46 // 35
    assert acc(p, 0, 1, T - 1, p, p, p, 0, 0, p, T, 5, 7, None) == 0
    with pytest.raises(DcunetError, match=r'\(-3\).*2\^46 = 70368744177664'):
        acc(p, 0, 1, T, p, p, p, 0, 0, p, T + 1, 5, 7, None)
    with pytest.raises(DcunetError, match=r'\(-3\).*2\^46 = 70368744177664'):
        acc(p, 1, 2, 2 ** 16 - 1, p, p, None, 1, 1, p, 2 ** 16 + 1, 2 ** 15, 2 ** 15, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
        fin(None, 4, p, 1, 4, p, p, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
        fin(p, 4, None, 1, 4, p, p, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
        fin(p, 4, p, -1, 4, p, p, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*ld = 3 is below T = 4'):
        fin(p, 3, p, 1, 4, p, p, None)
    with pytest.raises(DcunetError, match=r'\(-3\).*2\^46 = 70368744177664'):
        fin(p, 2 ** 46 + 1, p, 1, 2 ** 46 + 1, p, p, None)
    assert fin(p, 4, p, 0, 4, p, p, None) == 0 and fin(p, 4, p, 1, 4, None, None, None) == 0      # nothing to do: nothing launched


# ---- the traces file -----------------------------------------------------------------------------------------------------
def test_write_traces_dataset_is_the_spikes_models_schema(tmp_path):
    from deep_calcium_amd import hdf5_min, write_traces_dataset
    rs = np.random.RandomState(2)
    traces = rs.randn(5, 37).astype(np.float32)
    spikes = rs.rand(5, 37) > 0.9
    p = write_traces_dataset(str(tmp_path / 'a.hdf5'), traces, 'neurofinder.00.00', spikes=spikes)
    with hdf5_min.File(p) as f:
        name = f.attrs['name']
        assert (name.decode() if isinstance(name, bytes) else str(name)) == 'neurofinder.00.00'
        assert sorted(f.keys()) == ['spikes', 'traces']
        t, s = f['traces'].read(), f['spikes'].read()
        assert t.dtype == np.float32 and t.shape == (5, 37) and np.array_equal(t, traces)
        assert s.dtype == np.uint8 and np.array_equal(s, spikes.astype(np.uint8))
    p = write_traces_dataset(str(tmp_path / 'b.hdf5'), traces.astype(np.float64), 'x')
    with hdf5_min.File(p) as f:
        assert sorted(f.keys()) == ['traces'] and f['traces'].read().dtype == np.float64
    p = write_traces_dataset(str(tmp_path / 'c.npz'), np.arange(6).reshape(2, 3), 'exp-001', spikes=np.eye(2, 3))
    z = np.load(p, allow_pickle=False)
    assert sorted(z.files) == ['name', 'spikes', 'traces'] and str(z['name']) == 'exp-001'
    assert z['traces'].dtype.kind == 'i' and np.array_equal(z['traces'], np.arange(6).reshape(2, 3))
    assert z['spikes'].dtype == np.uint8 and np.array_equal(z['spikes'], np.eye(2, 3))
    for bad_traces, bad_spikes, what in ((np.zeros(4), None, r'\(R,T\)'), (traces, np.zeros((5, 36)), 'spikes are')):
        with pytest.raises(ValueError, match=what):
            write_traces_dataset(str(tmp_path / 'd.hdf5'), bad_traces, 'x', spikes=bad_spikes)


# ---- the 128-bit helpers ---------------------------------------------------------------------------------------------------
def test_trace_helpers_under_the_host_sanitizers(tmp_path):
    """dc_i128_add / dc_i128_from_i64 / dc_i128_mul_i64 of csrc/series_math.h compiled into tests/native/trace_math_check.cpp with
    the address and undefined-behaviour sanitizers and run as a program of its own."""
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
    exe = str(tmp_path / 'trace_math_check')
    src = os.path.join(ROOT, 'tests', 'native', 'trace_math_check.cpp')
    r = subprocess.run([cxx] + flags + [src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'trace_math_check: ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_frames_of_one_call_are_limited(dclib):
    """DC_FRAMES_PER_CALL_MAX: tc = 2^30 + 1 is refused with (-3) and the limit's message before any launch, tc = 2^30 is not."""
    import _wideindex
    _wideindex.check_frame_limit(dclib, 'test_traces_api')
