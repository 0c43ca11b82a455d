"""dF/F traces without a GPU: the public names and the ABI, neuropil_rois against a brute-force ring, the integer rank rule, the
coefficients of dc_trace_combine in Python big integers, argument validation in front of and inside the library, and the two
helpers of csrc/dff_math.h as a stand-alone program under the host sanitizers."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _dff_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_public_names_and_abi():
    import deep_calcium_amd
    from deep_calcium_amd import _build, _gen_tape, _lib, dff
    for name in ('TraceBaseline', 'neuropil_rois', 'dff_traces_device'):
        assert getattr(deep_calcium_amd, name) is getattr(dff, name) and name in deep_calcium_amd.__all__
    assert _lib.header_abi_version() >= 116 and 'dff.hip' in _build.SOURCES
    assert '-ffp-contract=off' in _build.FILE_FLAGS['dff.hip']
    protos = _lib.parse_header()
    tapeable = set(n for n, _ in _gen_tape.prototypes())
    for name in ('dc_trace_combine', 'dc_trace_baseline', 'dc_trace_scale'):
        assert name in protos and name in tapeable, name
    assert [len(protos[n][1]) for n in ('dc_trace_combine', 'dc_trace_baseline', 'dc_trace_scale')] == [10, 9, 7]
    header = open(_lib.HEADER).read()
    assert 'DC_TRACE_BASELINE_MAX_HALF 2047' in header and dff.MAX_HALF == 2047
    assert dff.KINDS == ('num', 'baseline_sum', 'f', 'baseline', 'dff')
    # new methods only: what the traces module offered stays what it was
    from deep_calcium_amd import traces
    assert traces.KINDS == ('sum', 'mean', 'zscore')
    assert callable(traces.RoiTraceExtractor.sums_device) and callable(traces.RoiTraceExtractor.areas_host)


def test_dff_module_imports_without_torch_or_the_library():
    code = ("import sys, deep_calcium_amd.dff as d; "
            "assert 'torch' not in sys.modules and 'deep_calcium_amd._lib' not in sys.modules; print(','.join(d.KINDS))")
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == 'num,baseline_sum,f,baseline,dff', out.stderr[-500:]


# ---- neuropil_rois -----------------------------------------------------------------------------------------------------------
def _same_rings(got, want):
    assert len(got) == len(want)
    for r, (g, w) in enumerate(zip(got, want)):
        assert g.ndim == 2 and g.shape[1] == 2 and g.dtype.kind == 'i', r
        assert np.array_equal(g, w), r                       # np.argwhere: raster order


def test_rings_equal_the_brute_force_ring():
    from deep_calcium_amd.dff import neuropil_rois
    from deep_calcium_amd.nf_metrics import mask_to_regions
    rs = np.random.RandomState(3)
    seen_empty = False
    for H, W, inner, outer in ((24, 24, 2, 12), (24, 17, 0, 1), (9, 24, 1, 3), (24, 24, 3, 4), (5, 5, 0, 64), (1, 7, 0, 2)):
        rois = []
        for _ in range(4):
            y, x = rs.randint(0, H), rs.randint(0, W)        # blobs anywhere: at the border, touching and overlapping included
            c = np.argwhere(np.ones((min(3, H - y), min(4, W - x)))) + [y, x]
            rois.append(c[rs.rand(len(c)) < 0.8] if len(c) > 2 else c)
        rois = [c for c in rois if len(c)]
        want = ref.rings(rois, (H, W), inner, outer)
        _same_rings(neuropil_rois(rois, (H, W), inner, outer), want)
        seen_empty = seen_empty or any(len(w) == 0 for w in want)
    assert seen_empty
    # the four input forms describe the same rings
    H, W = 20, 24
    mask = np.zeros((H, W), np.uint8)
    mask[0:3, 0:4] = 1                                       # at the image's corner
    mask[8:12, 8:12] = 1
    mask[8:12, 13:16] = 1                                    # one free column between this and the previous: their halos touch
    mask[19, 23] = 1
    regions = mask_to_regions(mask)
    assert len(regions) == 4
    stack = np.zeros((4, H, W), np.int8)
    for i, r in enumerate(regions):
        stack[i, r[:, 0], r[:, 1]] = 1
    dicts = [{'coordinates': [[int(y), int(x)] for y, x in r]} for r in regions]
    want = ref.rings(regions, (H, W), 2, 5)
    assert all(len(w) for w in want)
    for form in (mask, stack, dicts, [r[::-1] for r in regions]):
        _same_rings(neuropil_rois(form, (H, W), 2, 5), want)
    # no ring pixel is within `inner` of ANY ROI, the ROIs' own pixels included
    for ring in want:
        for c in regions:
            d = np.maximum(np.abs(ring[:, None, 0] - c[None, :, 0]), np.abs(ring[:, None, 1] - c[None, :, 1])).min(1)
            assert d.min() > 2


def test_touching_rois_and_an_empty_ring():
    from deep_calcium_amd.dff import neuropil_rois
    H, W = 12, 12
    # two ROIs that touch: the ring of each stays clear of the other
    a = np.argwhere(np.ones((3, 3))) + [4, 2]
    b = np.argwhere(np.ones((3, 3))) + [4, 5]
    got = neuropil_rois([a, b], (H, W), 1, 3)
    _same_rings(got, ref.rings([a, b], (H, W), 1, 3))
    assert len(got[0]) and len(got[1]) and got[0][:, 1].max() < 5 + 3 and not (set(map(tuple, got[0])) & set(map(tuple, b)))
    # an ROI fenced in by a neighbour that surrounds it: everything within `outer` of it is within `inner` of the fence
    centre = np.array([[6, 6]])
    fence = np.argwhere(np.ones((H, W)))
    fence = fence[np.maximum(np.abs(fence[:, 0] - 6), np.abs(fence[:, 1] - 6)) >= 2]
    got = neuropil_rois([centre, fence], (H, W), 1, 3)
    assert got[0].shape == (0, 2) and got[1].shape == (0, 2)
    _same_rings(got, ref.rings([centre, fence], (H, W), 1, 3))
    # an ROI that fills the image has nowhere to put a ring
    assert neuropil_rois(np.ones((1, 4, 5), np.int8), (4, 5))[0].shape == (0, 2)


# ---- the rank and the coefficients -----------------------------------------------------------------------------------------------
def test_integer_rank_rule_is_the_sorted_windows_index():
    from deep_calcium_amd.dff import rank_index
    differ = 0
    for n in range(1, 300):
        w = np.arange(n) * 3 + 7                             # distinct: the rank is visible in the value
        for q in range(101):
            k = rank_index(q, n)
            assert k == (q * (n - 1)) // 100 == ref.rank(q, n) and 0 <= k < n
            assert np.sort(w[::-1])[k] == 7 + 3 * k
            differ += int(k != int(np.floor(q / 100.0 * (n - 1))))
    assert rank_index(29, 101) == 29 and int(np.floor(0.29 * 100)) == 28 and differ > 0      # not numpy's float rule
    assert rank_index(0, 1) == 0 and rank_index(100, 4095) == 4094


def test_coefficients_give_the_headers_numerator_in_big_integers():
    from deep_calcium_amd.dff import combine_coefficients, weight_256ths
    assert [weight_256ths(w) for w in (0, 0.7, 0.75, 1, 0.5 / 256, 0.49 / 256)] == [0, 179, 192, 256, 1, 0]
    rs = np.random.RandomState(11)
    for weight, o in ((0.7, 0), (0.75, 100), (1.0, -65535), (0.0, 65535), (0.33, -7)):
        a = int(np.floor(256 * weight + 0.5))
        A = rs.randint(1, 2 ** 18, size=40)
        An = rs.randint(0, 2 ** 18, size=40)
        An[::5] = 0
        A[0], An[0] = 2 ** 18, 2 ** 18 - 1                   # just below the limit
        A[1], An[1] = 1, 2 ** 30
        ca, cb, cc, den, on = combine_coefficients(A, An, weight, o)
        assert all(x.dtype == np.int64 for x in (ca, cb, cc, den)) and np.array_equal(on, An > 0)
        for r in range(40):
            # the extremes of 16-bit pixels and something in between
            for S, Sn in ((65535 * int(A[r]), -32768 * int(An[r])), (-32768 * int(A[r]), 65535 * int(An[r])),
                          (int(rs.randint(-32768, 65536)) * int(A[r]), int(rs.randint(-32768, 65536)) * int(An[r]))):
                Ar, Anr = int(A[r]), int(An[r])
                if Anr > 0:
                    N, D = 256 * Anr * (S + o * Ar) - a * Ar * (Sn + o * Anr), 256 * Anr * Ar
                else:
                    N, D = S + o * Ar, Ar
                got = int(ca[r]) * S - int(cb[r]) * Sn + int(cc[r])
                assert got == N and int(den[r]) == D and abs(N) < 2 ** 62, (weight, o, r)
        wantN, wantD = ref.numerators(np.outer(A, [3, -2]), A, np.outer(An, [5, 1]), An, weight, o)
        assert np.array_equal(ca[:, None] * np.outer(A, [3, -2]) - cb[:, None] * np.outer(An, [5, 1]) + cc[:, None], wantN)
        assert np.array_equal(den, wantD)
    ca, cb, cc, den, on = combine_coefficients([4, 9], None, 0.7, 5)
    assert (ca.tolist(), cb.tolist(), cc.tolist(), den.tolist(), on.tolist()) == ([1, 1], [0, 0], [20, 45], [4, 9], [False, False])
    with pytest.raises(ValueError, match=r'ROI 1: .*2\*\*36'):
        combine_coefficients([5, 2 ** 18, 7], [5, 2 ** 18, 7])
    combine_coefficients([5, 2 ** 18, 7], [5, 2 ** 18 - 1, 7])


# ---- validation ----------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    from deep_calcium_amd import _lib, dff
    from deep_calcium_amd.dff import TraceBaseline, dff_traces_device, neuropil_rois

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'lib', boom)
    S = np.arange(12, dtype=np.int64).reshape(2, 6)
    A = [3, 4]
    for args, kw, what in (((S, A), dict(window=4), 'odd'),
                           ((S, A), dict(window=0), 'odd'),
                           ((S, A), dict(window=-3), 'odd'),
                           ((S, A), dict(window=3.0), 'integer'),
                           ((S, A), dict(window=4097), 'over the limit'),
                           ((S, A), dict(window=3, percentile=101), r'\[0, 100\]'),
                           ((S, A), dict(window=3, percentile=-1), r'\[0, 100\]'),
                           ((S, A), dict(window=3, percentile=8.5), 'integer'),
                           ((S, A), dict(window=3, weight=1.5, neuropil_sums=S, neuropil_areas=A), r'weight must be in \[0, 1\]'),
                           ((S, A), dict(window=3, weight=-0.1), r'weight must be in \[0, 1\]'),
                           ((S, A), dict(window=3, weight=float('nan')), r'weight must be in \[0, 1\]'),
                           ((S, A), dict(window=3, offset=65536), 'offset'),
                           ((S, A), dict(window=3, offset=-65536), 'offset'),
                           ((S, [3, 4, 5]), dict(window=3), 'areas'),
                           ((S, [3, 0]), dict(window=3), 'areas'),
                           ((S, [3.0, 4.0]), dict(window=3), 'areas'),
                           ((S.astype(np.int32), A), dict(window=3), 'int64'),
                           ((S[0], A), dict(window=3), 'int64'),
                           ((S.tolist(), A), dict(window=3), 'numpy array or a device tensor'),
                           ((S, A), dict(window=3, neuropil_sums=S), 'together'),
                           ((S, A), dict(window=3, neuropil_areas=A), 'together'),
                           ((S, A), dict(window=3, neuropil_sums=S[:, :5], neuropil_areas=A), 'neuropil_sums is'),
                           ((S, A), dict(window=3, neuropil_sums=S, neuropil_areas=[1, 2, 3]), 'neuropil_areas'),
                           ((S, A), dict(window=3, neuropil_sums=S, neuropil_areas=[1, -2]), 'neuropil_areas'),
                           ((S, [2 ** 18, 4]), dict(window=3, neuropil_sums=S, neuropil_areas=[2 ** 18, 4]), r'ROI 0: .*2\*\*36')):
        with pytest.raises(ValueError, match=what):
            TraceBaseline(*args, **kw)
    ok = [np.array([[1, 2], [3, 4]])]
    for kw, what in ((dict(inner=3, outer=3), 'inner < outer'), (dict(inner=4, outer=2), 'inner < outer'), (dict(inner=-1, outer=2), 'inner < outer'),
                     (dict(inner=2, outer=65), 'inner < outer'), (dict(inner=1.5, outer=3), 'integer')):
        with pytest.raises(ValueError, match=what):
            neuropil_rois(ok, (8, 8), **kw)
    with pytest.raises(ValueError, match='outside'):
        neuropil_rois([np.array([[8, 0]])], (8, 8))
    with pytest.raises(ValueError, match='shape'):
        neuropil_rois(ok, (8,))
    # the streaming front end: refused before the file is even opened
    nowhere = '/nonexistent/dataset.npz'
    for kw, what in ((dict(window=10), 'odd'), (dict(window=4097), 'over the limit'), (dict(window=3, percentile=101), r'\[0, 100\]'),
                     (dict(window=3, kind='median'), 'not one of'), (dict(window=3, kind='zscore'), 'not one of'),
                     (dict(window=3, offset=10 ** 6), 'offset'), (dict(window=3, neuropil=(2, 12)), 'inner, outer, weight'),
                     (dict(window=3, neuropil=(12, 2, 0.7)), 'inner < outer'), (dict(window=3, neuropil=(2, 12, 1.5)), 'weight'),
                     (dict(window=3, shifts=np.zeros((4, 2), int), fine_shifts=np.zeros((4, 2), int)), 'not both')):
        with pytest.raises(ValueError, match=what):
            dff_traces_device(nowhere, ok, **kw)
    assert dff.window_half(1) == 0 and dff.window_half(4095) == 2047


def test_c_abi_argument_validation_returns_codes(dclib):
    """Refused before any launch (there is no GPU here): the pointers are never followed."""
    from deep_calcium_amd._lib import DcunetError
    p = 4096                                  # any aligned non-null value
    com, bas, sca = dclib.dc_trace_combine, dclib.dc_trace_baseline, dclib.dc_trace_scale
    ok = [p, 8, p, p, p, p, 2, 8, p, None]
    for i in (0, 2, 3, 4, 5, 8):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            com(*[None if j == i else a for j, a in enumerate(ok)])
    for i in (0, 3, 4, 5, 8):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            com(*[a + 4 if j == i else a for j, a in enumerate(ok)])
    with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
        com(p, 8, p + 2, p, p, p, 2, 8, p, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*ld = 7 is below T = 8'):
        com(p, 7, p, p, p, p, 2, 8, p, None)
    for R, T in ((-1, 8), (2, -1)):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
            com(p, 8, p, p, p, p, R, T, p, None)
    assert com(p, 8, p, p, p, p, 0, 8, p, None) == 0 and com(p, 8, p, p, p, p, 2, 0, p, None) == 0      # nothing to do: nothing launched

    with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
        bas(None, 8, 2, 8, 3, 8, p, p, None)
    with pytest.raises(DcunetError, match=r'\(-3\).*half = 2048.*2047'):
        bas(p, 8, 2, 8, 2048, 8, p, p, None)
    for q in (-1, 101):
        with pytest.raises(DcunetError, match=r'\(-1\).*q = %d' % q):
            bas(p, 8, 2, 8, 3, q, p, p, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*ld = 7 is below T = 8'):
        bas(p, 7, 2, 8, 3, 8, p, p, None)
    for R, T, half in ((-1, 8, 3), (2, -1, 3), (2, 8, -1)):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
            bas(p, max(T, 0), R, T, half, 8, p, p, None)
    for args in ((p + 4, 8, 2, 8, 3, 8, p, p, None), (p, 8, 2, 8, 3, 8, p + 4, p, None), (p, 8, 2, 8, 3, 8, p, p + 2, None)):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            bas(*args)
    assert bas(p, 8, 0, 8, 3, 8, p, p, None) == 0 and bas(p, 8, 2, 0, 3, 8, p, p, None) == 0
    assert bas(p, 8, 2, 8, 2047, 100, None, None, None) == 0                       # neither output: nothing launched

    for args in ((None, 8, p, 2, 8, p, None), (p, 8, None, 2, 8, p, None), (p, 8, p, 2, 8, None, None)):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            sca(*args)
    with pytest.raises(DcunetError, match=r'\(-1\).*ld = 7 is below T = 8'):
        sca(p, 7, p, 2, 8, p, None)
    for R, T in ((-1, 8), (2, -1)):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
            sca(p, 8, p, R, T, p, None)
    for args in ((p + 4, 8, p, 2, 8, p, None), (p, 8, p + 4, 2, 8, p, None), (p, 8, p, 2, 8, p + 2, None)):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            sca(*args)
    assert sca(p, 8, p, 0, 8, p, None) == 0 and sca(p, 8, p, 2, 0, p, None) == 0


# ---- the helpers of the kernel ---------------------------------------------------------------------------------------------------
def test_dff_helpers_under_the_host_sanitizers(tmp_path):
    """dc_dff_rank / dc_dff_midpoint of csrc/dff_math.h compiled into tests/native/dff_math_check.cpp with the address and
    undefined-behaviour sanitizers and run as a program of its own: the midpoint at the int64 extremes, the rank at its limits."""
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
    exe = str(tmp_path / 'dff_math_check')
    src = os.path.join(ROOT, 'tests', 'native', 'dff_math_check.cpp')
    r = subprocess.run([cxx] + flags + [src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'dff_math_check: ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
