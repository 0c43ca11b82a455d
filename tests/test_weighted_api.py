"""Weighted ROI traces without a GPU: the public names and the ABI, the entry point's argument checks (they precede any launch),
every ValueError in front of the library, footprint_weights / exclude_overlap / roi_gram / demix_traces against the plain loops of
tests/_weighted_ref.py, the reach table on the exact integer oracle (two overlapping cells: binary sums carry the neighbour,
excluding or demixing the shared pixels removes it), and csrc/wtrace_math.h as a stand-alone program under the host sanitizers."""
import inspect
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _weighted_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('WeightedTraceExtractor', 'weighted_traces_device', 'footprint_weights', 'exclude_overlap', 'roi_gram', 'demix_traces')


def test_public_names_and_abi():
    import deep_calcium_amd
    from deep_calcium_amd import _build, _gen_tape, _lib, dff, traces, weighted
    for name in NAMES:
        assert getattr(deep_calcium_amd, name) is getattr(weighted, name) and name in deep_calcium_amd.__all__
    assert _lib.header_abi_version() >= 125
    protos = _lib.parse_header()
    assert 'dc_roi_wtrace_accumulate' in protos and 'dc_roi_wtrace_accumulate' in set(n for n, _ in _gen_tape.prototypes())
    assert len(protos['dc_roi_wtrace_accumulate'][1]) == len(protos['dc_roi_trace_accumulate'][1]) + 1 == 15
    assert protos['dc_roi_wtrace_accumulate'][2][6] == 'row_wgt'
    assert open(_gen_tape.OUT).read() == _gen_tape.render()                 # the committed trampolines are current
    assert 'Weighted ROI traces' in open(_lib.HEADER).read()
    assert '-ffp-contract=off' in _build.FILE_FLAGS['traces.hip']
    assert issubclass(weighted.WeightedTraceExtractor, traces.RoiTraceExtractor)
    assert list(inspect.signature(weighted.WeightedTraceExtractor.__init__).parameters)[1:] == [
        'shape', 'n_frames', 'dtype', 'rois', 'weights', 'device', 'chunk_frames', 'shifts', 'fine_shifts', 'bidi']
    assert inspect.signature(dff.dff_traces_device).parameters['weights'].default is None
    sig = inspect.signature(weighted.weighted_traces_device).parameters
    assert sig['weights'].default is None and sig['kind'].default == 'mean' and sig['overlap'].default == 'keep'
    assert weighted.MAX_WSUM == 2 ** 31 - 1 and weighted.MAX_VOLUME == 2 ** 46 and weighted.MAX_COMPONENT == 64
    math_h = open(os.path.join(ROOT, 'deep_calcium_amd', 'csrc', 'wtrace_math.h')).read()
    assert '#define DC_WTRACE_MAX_WSUM 2147483647L' in math_h and '#define DC_WTRACE_MAX_VOLUME 70368744177664L' in math_h


def test_the_library_exports_the_entry_point_and_checks_its_arguments_without_a_device(dclib):
    c = dclib.cdll
    assert dclib.cdll.dc_version() >= 125
    f = c.dc_roi_wtrace_accumulate
    P = 4096                     # any non-null, 16-byte aligned value: every call below must fail before a launch

    def call(frames=P, uns=0, tc=4, t0=0, off=P, pix=P, wgt=P, roi=P, S=3, R=2, sums=P, ld=8, H=5, W=7):
        return f(frames, uns, tc, t0, off, pix, wgt, roi, S, R, sums, ld, H, W, None)

    def rejected(rc, code, word):
        assert rc == code and word in c.dc_last_error().decode() and 'dc_roi_wtrace_accumulate' in c.dc_last_error().decode(), \
            (rc, c.dc_last_error())

    for kw in (dict(frames=None), dict(off=None), dict(pix=None), dict(wgt=None), dict(sums=None)):
        rejected(call(**kw), -1, 'null pointer')
    for kw in (dict(S=-1), dict(R=-1), dict(tc=-1), dict(t0=-1)):
        rejected(call(**kw), -1, 'negative count')
    rejected(call(roi=None, S=3, R=2), -1, 'without row_roi')
    rejected(call(ld=3), -1, 'ld = 3')
    rejected(call(t0=5, tc=4, ld=8), -1, 'ld = 8')
    for kw in (dict(H=0), dict(W=0), dict(H=2 ** 15 + 1, W=2 ** 15)):
        rejected(call(**kw), -1, 'out of range')
    for kw in (dict(wgt=P + 1), dict(frames=P + 1), dict(off=P + 2), dict(pix=P + 2), dict(roi=P + 2), dict(sums=P + 4)):
        rejected(call(**kw), -1, 'misaligned')
    rejected(call(H=2 ** 15, W=2 ** 15, tc=1, t0=2 ** 16, ld=2 ** 17), -3, '2^46')
    # nothing to do: no launch, no error (the unweighted entry point's rule)
    assert call(tc=0) == 0 and call(R=0, S=0, roi=None) == 0
    # the unweighted entry point shares the checks and keeps its own name in the message
    g = c.dc_roi_trace_accumulate
    rc = g(None, 0, 4, 0, P, P, P, 3, 2, P, 8, 5, 7, None)
    assert rc == -1 and 'dc_roi_trace_accumulate: null pointer' in c.dc_last_error().decode()


def test_module_imports_without_torch_or_the_library():
    code = ("import sys, deep_calcium_amd.weighted as m; "
            "assert 'torch' not in sys.modules and 'deep_calcium_amd._lib' not in sys.modules; print(','.join(m.OVERLAPS))")
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == 'keep,exclude,demix', out.stderr[-500:]


# ---- every ValueError -----------------------------------------------------------------------------------------------------------------
SQUARE = np.array([[1, 1], [1, 2], [2, 1], [2, 2]])
PAIR = np.array([[1, 3], [2, 3]])


def test_arguments_are_checked_before_the_library_is_touched(monkeypatch, tmp_path):
    from deep_calcium_amd import _lib, dff, weighted
    X = weighted.WeightedTraceExtractor

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'lib', boom)
    monkeypatch.setitem(sys.modules, 'torch', None)                          # `import torch` raises ImportError from here on
    rois = [SQUARE, PAIR]
    ok = [np.array([1, 2, 3, 4]), np.array([5, 6])]
    big = np.array([[y, x] for y in range(200) for x in range(200)])          # 40000 pixels
    cases = ((rois, [ok[0], np.array([5, 6, 7])], 8, 'ROI 1 has 2 pixels and 3 weights'),
             (rois, [ok[0]], 8, 'one per ROI'),
             (rois, None, 8, 'weights must be'),
             ([np.array([[1, 1], [2, 2], [1, 1]]), PAIR], [np.array([1, 2, 3]), ok[1]], 8, r'ROI 0 lists the pixel \[1, 1\] more than once'),
             (rois, [ok[0], np.array([5.0, 6.0])], 8, 'ROI 1: weights must be integers'),
             (rois, [ok[0], np.array([True, False])], 8, 'ROI 1: weights must be integers'),
             (rois, [np.array([1, 2, 3, 65536]), ok[1]], 8, r'ROI 0: a weight is outside \[0, 65535\]'),
             (rois, [np.array([1, -1, 3, 4]), ok[1]], 8, 'ROI 0: a weight is outside'),
             (rois, [ok[0], np.array([0, 0])], 8, 'ROI 1: its weights sum to 0'),
             ([SQUARE, big], [ok[0], np.full(40000, 65535)], 8, r'ROI 1: its weights sum to 2621400000, more than 2\*\*31 - 1'),
             (rois, [ok[0], np.array([65535, 65535])], 2 ** 30, r'ROI 1: n_frames \* weight sum = 1073741824 \* 131070 exceeds 2\*\*46'),
             ([SQUARE, np.zeros((0, 2), np.int64)], [ok[0], np.zeros(0, np.int64)], 8, 'ROI 1 is empty'),
             ([SQUARE, np.array([[1, 7]])], [ok[0], np.array([1])], 8, 'ROI 1 has a coordinate outside'),
             (np.zeros((5, 7), np.int32), ok, 8, 'rois must be a list'))
    for r, w, T, what in cases:
        with pytest.raises(ValueError, match=what):
            X((300, 300) if r[-1] is big else (5, 7), T, np.int16, r, w)
    for kw, what in ((dict(chunk_frames=0), 'chunk_frames'), (dict(bidi=7), 'bidi'), (dict(shifts=np.zeros((7, 2), np.int32)), 'shifts')):
        with pytest.raises(ValueError, match=what):
            X((5, 7), 8, np.int16, rois, ok, **kw)
    with pytest.raises(ValueError, match='n_frames'):
        X((5, 7), 0, np.int16, rois, ok)
    with pytest.raises(ValueError, match='int16 or uint16'):
        X((5, 7), 8, np.float32, rois, ok)
    # the limits themselves are served as far as the arguments go: W just below 2^31, T W = 2^46 exactly
    entries = weighted._weighted_entries([big], [np.full(40000, 53687)], (300, 300))
    assert weighted._check_wsums(entries, 1).tolist() == [40000 * 53687]
    assert weighted._check_wsums(weighted._weighted_entries([PAIR], [np.array([2 ** 15, 2 ** 15])], (5, 7)), 2 ** 30).tolist() == [2 ** 16]
    # the one-call functions
    path = str(tmp_path / 'recording.npz')
    np.savez(path, series_raw=np.zeros((8, 5, 7), np.int16))
    W = weighted.weighted_traces_device
    for kw, what in ((dict(overlap='drop'), 'overlap'), (dict(kind='median'), 'kind'), (dict(overlap='demix', kind='mean'), "'demix' or 'zscore'"),
                     (dict(kind='demix'), 'kind'), (dict(bidi=1.5), 'bidi'),
                     (dict(shifts=np.zeros((8, 2), np.int32), fine_shifts=np.zeros((8, 2), np.int32)), 'not both')):
        with pytest.raises(ValueError, match=what):
            W('/nonexistent/dataset.npz', rois, ok, **kw)
    with pytest.raises(ValueError, match='ROI 1: its weights sum to 0'):
        W(path, rois, [ok[0], np.array([0, 0])])
    with pytest.raises(ValueError, match='ROI 1 has no pixel of its own left'):
        W(path, [SQUARE, np.array([[1, 1], [2, 2]])], None, overlap='exclude')
    with pytest.raises(ValueError, match=r'ROIs \[0, 1\] have linearly dependent footprints'):
        W(path, [SQUARE, SQUARE[::-1]], None, kind='demix', overlap='demix')
    with pytest.raises(ValueError, match='ROI 0: a weight is outside'):
        dff.dff_traces_device(path, rois, 5, weights=[np.array([1, 2, 3, 70000]), ok[1]])
    with pytest.raises(ValueError, match='ROI 1 has 2 pixels and 1 weights'):
        dff.dff_traces_device(path, rois, 5, neuropil=(1, 3, 0.7), weights=[ok[0], np.array([3])])


def test_inside_the_limits_the_arguments_reach_the_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present')
    from deep_calcium_amd import WeightedTraceExtractor
    from deep_calcium_amd._lib import DcunetError
    with pytest.raises(DcunetError, match='no CPU fallback'):
        WeightedTraceExtractor((5, 7), 8, np.uint16, [SQUARE, PAIR], [np.array([0, 65535, 3, 4]), np.array([5, 6])])


# ---- the rules on the host ----------------------------------------------------------------------------------------------------------
def _same_lists(got_r, got_w, want_r, want_w):
    assert [np.asarray(c).tolist() for c in got_r] == [list(map(list, c)) for c in want_r]
    assert [np.asarray(w).tolist() for w in got_w] == [list(w) for w in want_w]


def test_footprint_weights_on_hand_made_maps_equals_the_plain_loops():
    from deep_calcium_amd import footprint_weights
    nan = float('nan')
    coords = [np.array([[0, 0], [0, 1], [1, 0], [1, 1], [2, 2]]), np.array([[3, 3], [3, 4]]), np.array([[4, 4], [4, 5], [4, 6]])]
    corr = [np.array([1.0, 0.5, -0.3, nan, 0.001], np.float32), np.array([nan, -1.0], np.float32), np.array([0.3, 0.29999, 1.5], np.float64)]
    inside = [np.array([1, 1, 1, 1, 0], bool), np.array([1, 1], bool), np.array([0, 1, 1], bool)]
    for ins in (None, inside):
        for floor in (0.0, 0.3, -1.0, 0.0019):
            r, w, k = footprint_weights(coords, corr, inside=ins, floor=floor)
            rr, ww, kk = ref.footprint_weights(coords, corr, ins, floor)
            assert k == kk
            _same_lists(r, w, rr, ww)
    r, w, k = footprint_weights(coords, corr)
    assert k == [0, 2] and [a.tolist() for a in w] == [[256, 128], [77, 77, 256]] and r[0].tolist() == [[0, 0], [0, 1]]      # 0.001 -> 0; 1.5 -> 256
    assert all(a.dtype == np.int64 for a in r + w)
    # the rounding: half up, in float64
    v = np.array([0.5 / 256, 0.49999 / 256, 1.5 / 256, 255.5 / 256, 255.49 / 256])
    assert footprint_weights([np.array([[0, i] for i in range(5)])], [v])[1][0].tolist() == [1, 2, 256, 255]
    assert [ref.weight_of(x) for x in v] == [1, 0, 2, 256, 255]
    rs = np.random.RandomState(11)
    for trial in range(30):
        n = rs.randint(1, 5)
        cs = [np.stack([rs.permutation(30)[:k] // 6, rs.permutation(30)[:k] % 6], 1) for k in rs.randint(1, 12, n)]
        vs = [np.where(rs.rand(len(c)) < 0.1, nan, rs.uniform(-0.5, 1.0, len(c))).astype(np.float32) for c in cs]
        ins = [rs.rand(len(c)) < 0.7 for c in cs]
        floor = float(rs.choice([0.0, 0.2, 0.6]))
        r, w, k = footprint_weights(cs, vs, inside=ins, floor=floor)
        rr, ww, kk = ref.footprint_weights(cs, vs, ins, floor)
        assert k == kk
        _same_lists(r, w, rr, ww)
    with pytest.raises(ValueError, match='floor'):
        footprint_weights(coords, corr, floor=nan)
    with pytest.raises(ValueError, match='3 supports, 2 maps'):
        footprint_weights(coords, corr[:2])
    with pytest.raises(ValueError, match='ROI 1: inside'):
        footprint_weights(coords, corr, inside=[inside[0], np.array([1, 1]), inside[2]])


def test_exclude_overlap_and_gram_with_a_pixel_shared_by_three_rois():
    from deep_calcium_amd import exclude_overlap, roi_gram
    from deep_calcium_amd.weighted import shared_pixels
    a = np.array([[1, 1], [1, 2], [2, 2], [0, 0]])                         # (1,2) shared by all three, (2,2) by a and b
    b = np.array([[2, 2], [1, 2], [3, 3]])
    c = np.array([[1, 2], [4, 4]])
    d = np.array([[1, 2]])                                                # nothing of its own: dropped
    w = [np.array([10, 20, 30, 40]), np.array([5, 6, 7]), np.array([65535, 1]), np.array([9])]
    rois = [a, b, c, d]
    assert shared_pixels(rois, (5, 6)) == 2
    r, ww, kept = exclude_overlap(rois, (5, 6), w)
    rr, rw, rk = ref.exclude_overlap(rois, w)
    assert kept == rk == [0, 1, 2]
    _same_lists(r, ww, rr, rw)
    assert [x.tolist() for x in r] == [[[0, 0], [1, 1]], [[3, 3]], [[4, 4]]] and [x.tolist() for x in ww] == [[40, 10], [7], [1]]
    r1, w1, k1 = exclude_overlap(rois, (5, 6))
    assert w1 is None and k1 == kept and [x.tolist() for x in r1] == [x.tolist() for x in r]
    G = roi_gram(rois, w, (5, 6))
    assert G.dtype == np.int64 and G.tolist() == ref.gram(rois, w) and np.array_equal(G, G.T)
    assert np.diag(G).tolist() == [int((x.astype(np.int64) ** 2).sum()) for x in w]
    assert G[0, 1] == 20 * 6 + 30 * 5 and G[0, 2] == 20 * 65535 and G[2, 3] == 65535 * 9 and G[2, 2] == 65535 ** 2 + 1
    assert roi_gram(rois, None, (5, 6)).tolist() == ref.gram(rois) == [[4, 2, 1, 1], [2, 3, 1, 1], [1, 1, 2, 1], [1, 1, 1, 1]]
    rs = np.random.RandomState(5)
    for trial in range(20):
        n = rs.randint(1, 6)
        cs = [np.stack(np.divmod(rs.permutation(24)[:k], 6), 1) for k in rs.randint(1, 10, n)]
        ws = [rs.randint(0, 65536, len(x)) for x in cs]
        assert roi_gram(cs, ws, (4, 6)).tolist() == ref.gram(cs, ws)
        r, ww, kept = exclude_overlap(cs, (4, 6), ws)
        rr, rw, rk = ref.exclude_overlap(cs, ws)
        assert kept == rk
        _same_lists(r, ww, rr, rw)
    with pytest.raises(ValueError, match='ROI 1 lists the pixel'):
        exclude_overlap([a, np.array([[1, 1], [1, 1]])], (5, 6))


def test_demix_traces_against_exact_rationals_and_its_refusals():
    from deep_calcium_amd import demix_traces, roi_gram
    from deep_calcium_amd.weighted import bareiss_determinant
    rs = np.random.RandomState(8)
    # disjoint ROIs: S / G_ii, bit for bit
    rois = [np.array([[0, 0], [0, 1]]), np.array([[1, 0]]), np.array([[2, 2], [2, 3], [3, 3]])]
    w = [np.array([3, 4]), np.array([256]), np.array([1, 2, 2])]
    G = roi_gram(rois, w, (4, 4))
    assert G.tolist() == [[25, 0, 0], [0, 65536, 0], [0, 0, 9]]
    S = rs.randint(-2 ** 40, 2 ** 40, size=(3, 17))
    assert np.array_equal(demix_traces(S, G), S.astype(np.float64) / np.diag(G).astype(np.float64)[:, None])
    # overlapping groups, one of three and one of two, and a singleton between them
    rois = [np.array([[0, 0], [0, 1], [0, 2]]), np.array([[0, 2], [0, 3]]), np.array([[3, 3]]), np.array([[0, 3], [1, 3]]),
            np.array([[2, 0], [2, 1]]), np.array([[2, 1], [3, 1]])]
    w = [np.array([200, 256, 90]), np.array([120, 250]), np.array([7]), np.array([60, 256]), np.array([256, 100]), np.array([100, 256])]
    G = roi_gram(rois, w, (4, 4))
    assert ref.components(G.tolist()) == [[0, 1, 3], [2], [4, 5]]
    truth = rs.randint(-5000, 5000, size=(6, 23))
    S = (G @ truth).astype(np.int64)                                       # S = G c with integer c: the exact answer is c itself
    got = demix_traces(S, G)
    want = ref.demix(S, G.tolist())
    assert np.array_equal(want, truth.astype(np.float64))
    assert got.dtype == np.float64 and np.allclose(got, want, rtol=1e-12, atol=1e-9)
    S2 = rs.randint(-2 ** 45, 2 ** 45, size=(6, 9))
    got2, want2 = demix_traces(S2, G), ref.demix(S2, G.tolist())
    assert np.abs(got2 - want2).max() <= 1e-12 * np.abs(want2).max()
    # Bareiss against the rationals' verdict
    assert bareiss_determinant([[2, 1], [1, 3]]) == 5 and bareiss_determinant([[0, 1], [1, 0]]) == -1 and bareiss_determinant([[7]]) == 7
    assert bareiss_determinant([[1, 2, 3], [4, 5, 6], [7, 8, 9]]) == 0 and bareiss_determinant([[0, 0], [0, 5]]) == 0
    for trial in range(30):
        n = rs.randint(1, 7)
        M = rs.randint(-2 ** 40, 2 ** 40, size=(n, n)).tolist()
        assert bareiss_determinant(M) == _det_fraction(M), trial
    # identical footprints: determinant 0, the ROIs are named
    same = [np.array([[0, 0], [0, 1]]), np.array([[2, 2]]), np.array([[0, 1], [0, 0]])]
    Gs = roi_gram(same, [np.array([5, 9]), np.array([1]), np.array([9, 5])], (3, 3))
    with pytest.raises(ValueError, match=r'ROIs \[0, 2\] have linearly dependent footprints'):
        demix_traces(np.zeros((3, 4), np.int64), Gs)
    assert ref.solve_exact([[Gs[0, 0], Gs[0, 2]], [Gs[2, 0], Gs[2, 2]]], [[1], [2]]) is None
    # a chain of 65 ROIs, each sharing one pixel with the next: one component too large; 64 are served
    chain = [np.array([[0, i], [0, i + 1]]) for i in range(65)]
    Gc = roi_gram(chain, None, (1, 66))
    with pytest.raises(ValueError, match='one group of 65: more than 64'):
        demix_traces(np.zeros((65, 2), np.int64), Gc)
    S64 = rs.randint(-1000, 1000, size=(64, 3))
    assert np.allclose(demix_traces(S64, Gc[:64, :64]), ref.demix(S64, Gc[:64, :64].tolist()), rtol=1e-9, atol=1e-9)
    for bad_s, bad_g, what in ((np.zeros((3, 4)), Gs, 'sums must be'), (np.zeros((2, 4), np.int64), Gs, 'gram must be'),
                               (np.zeros((2, 4), np.int64), np.array([[1, 2], [3, 4]]), 'symmetric')):
        with pytest.raises(ValueError, match=what):
            demix_traces(bad_s, bad_g)


def _det_fraction(M):
    """The determinant over the rationals (plain Gaussian elimination on Fractions)."""
    from fractions import Fraction
    m = [[Fraction(v) for v in row] for row in M]
    n, det = len(m), Fraction(1)
    for k in range(n):
        piv = next((i for i in range(k, n) if m[i][k] != 0), None)
        if piv is None:
            return 0
        if piv != k:
            m[k], m[piv] = m[piv], m[k]
            det = -det
        det *= m[k][k]
        for i in range(k + 1, n):
            f = m[i][k] / m[k][k]
            m[i] = [a - f * b for a, b in zip(m[i], m[k])]
    assert det.denominator == 1
    return int(det)


def test_oracle_sums_are_numpy_on_small_numbers():
    rs = np.random.RandomState(2)
    for dtype in (np.int16, np.uint16):
        info = np.iinfo(dtype)
        frames = rs.randint(info.min, info.max + 1, size=(5, 4, 6)).astype(dtype)
        rois = [np.stack(np.divmod(rs.permutation(24)[:k], 6), 1) for k in (5, 1, 9)]
        w = [rs.randint(0, 65536, len(c)) for c in rois]
        want = np.stack([(frames[:, c[:, 0], c[:, 1]].astype(np.int64) * x[None]).sum(1) for c, x in zip(rois, w)])
        assert np.array_equal(ref.roi_sums(frames, rois, w), want)
        off = np.concatenate([[0], np.cumsum([len(c) for c in rois])])
        pix = np.concatenate([c[:, 0] * 6 + c[:, 1] for c in rois])
        assert ref.csr_sums(frames, off, pix, np.concatenate(w), None, 3) == want.tolist()
        assert ref.csr_sums(frames, off, pix, np.concatenate(w), [2, 5, 2], 3) == [[0] * 5, [0] * 5, (want[0] + want[2]).tolist()]


# ---- the reach of the rules, on the exact oracle ---------------------------------------------------------------------------------
SEEDS = range(20)
METHODS = ('binary', 'exclude', 'weighted', 'binary + demix', 'weighted + demix')


def test_reach_table_shared_pixels_carry_the_neighbour_and_demixing_removes_it():
    """_weighted_ref.scene(seed), seeds 0..19: two Gaussian cells (radius 3.2) five pixels apart in a 12 x 20 frame, T = 1024,
    amplitude 60, sigma 30, shared neuropil at 0.3; the ROIs are the pixels above 0.2 of each peak and share 16 pixels.  The sums
    are the oracle's exact integers standing in for the device, the weights footprint_weights of the oracle's exact footprint
    correlations (the pixel's own series taken out of its ROI's trace), the demix demix_traces.  Printed: min / max / mean over the
    seeds of corr(trace of ROI 1, truth 1) and corr(trace of ROI 1, truth 2)."""
    from deep_calcium_amd import demix_traces, exclude_overlap, footprint_weights, roi_gram
    own = dict((m, []) for m in METHODS)
    cross = dict((m, []) for m in METHODS)
    for seed in SEEDS:
        frames, rois, truth = ref.scene(seed)
        shared = set(map(tuple, rois[0].tolist())) & set(map(tuple, rois[1].tolist()))
        assert len(shared) == 16
        corr = [ref.inside_corr(frames, r) for r in rois]
        wr, ww, kept = footprint_weights(rois, corr, inside=[np.ones(len(r), bool) for r in rois])
        assert kept == [0, 1]
        xr, _, xk = exclude_overlap(rois, ref.SHAPE)
        assert xk == [0, 1]
        f64 = frames.astype(np.int64)

        def sums(rs_, ws_):
            return np.stack([(f64[:, c[:, 0], c[:, 1]] * (np.ones(len(c), np.int64) if ws_ is None else np.asarray(ws_[i]))[None]).sum(1)
                             for i, c in enumerate(rs_)])
        B, X, Wt = sums(rois, None), sums(xr, None), sums(wr, ww)
        traces = {'binary': B[0], 'exclude': X[0], 'weighted': Wt[0],
                  'binary + demix': demix_traces(B, roi_gram(rois, None, ref.SHAPE))[0],
                  'weighted + demix': demix_traces(Wt, roi_gram(wr, ww, ref.SHAPE))[0]}
        for m in METHODS:
            own[m].append(ref.pearson(traces[m], truth[0]))
            cross[m].append(ref.pearson(traces[m], truth[1]))
    print('%-18s %-26s %-26s' % ('', 'corr with its own cell', 'corr with the other cell'))
    print('%-18s %8s %8s %8s %8s %8s %8s' % ('', 'min', 'max', 'mean', 'min', 'max', 'mean'))
    for m in METHODS:
        print('%-18s %8.3f %8.3f %8.3f %8.3f %8.3f %8.3f' % (m, min(own[m]), max(own[m]), np.mean(own[m]), min(cross[m]), max(cross[m]),
                                                             np.mean(cross[m])))
    mean_cross = dict((m, float(np.mean(cross[m]))) for m in METHODS)
    mean_abs = dict((m, abs(mean_cross[m])) for m in METHODS)
    assert mean_cross['binary'] >= 2 * mean_abs['exclude']
    assert mean_cross['binary'] >= 4 * mean_abs['weighted + demix']
    assert np.mean(own['weighted + demix']) > np.mean(own['binary'])


# ---- the scalar arithmetic of the kernel -------------------------------------------------------------------------------------------
def test_wtrace_math_under_the_host_sanitizers(tmp_path):
    """csrc/wtrace_math.h compiled into tests/native/wtrace_math_check.cpp with the address and undefined-behaviour sanitizers and
    run as a program of its own: one term against __int128, what 32 bits hold of it, a row at the bound summed in the kernel's
    order, and the promises made of a weight sum that stands for an area."""
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
    exe = str(tmp_path / 'wtrace_math_check')
    src = os.path.join(ROOT, 'tests', 'native', 'wtrace_math_check.cpp')
    r = subprocess.run([cxx] + flags + [src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'wtrace_math_check: ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_frames_of_one_call_are_limited(dclib):
    """DC_FRAMES_PER_CALL_MAX: tc = 2^30 + 1 is refused with (-3) and the limit's message before any launch, tc = 2^30 is not."""
    import _wideindex
    _wideindex.check_frame_limit(dclib, 'test_weighted_api')
