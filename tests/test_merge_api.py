"""Merging fragmented ROIs without a GPU: the public names and the ABI, roi_neighbours against brute force, every ValueError in
front of the library, the merge rule against the flood fill of tests/_merge_ref.py, the reach table on the exact integer oracle
(bleaching merges distinct cells; detrending parts them again), and csrc/trace_pair_math.h as a stand-alone program under the host
sanitizers."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _merge_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES = ('dc_trace_pair_moments', 'dc_trace_pair_corr')


def test_public_names_and_abi():
    import deep_calcium_amd
    from deep_calcium_amd import _build, _gen_tape, _lib, merge
    for name in ('TracePairCorr', 'roi_neighbours', 'merge_rois', 'merge_rois_device'):
        assert getattr(deep_calcium_amd, name) is getattr(merge, name) and name in deep_calcium_amd.__all__
    assert _lib.header_abi_version() >= 123 and 'trace_pairs.hip' in _build.SOURCES
    assert '-ffp-contract=off' in _build.FILE_FLAGS['trace_pairs.hip']
    protos = _lib.parse_header()
    tapeable = set(n for n, _ in _gen_tape.prototypes())
    for name in LAUNCHES:
        assert name in protos and name in tapeable, name
    assert [len(protos[n][1]) for n in LAUNCHES] == [9, 4]
    header = open(_lib.HEADER).read()
    assert 'ROI trace-pair correlation' in header
    assert '#define DC_TRACE_PAIR_MAX_PAIRS 16777216L' in header and merge.MAX_PAIRS == 2 ** 24 and merge.MAX_DIST == 16
    assert merge.KINDS == ('moments', 'corr')
    for f in ('trace_pairs.hip', 'trace_pair_math.h'):
        assert '#pragma clang fp contract(off)' in open(os.path.join(ROOT, 'deep_calcium_amd', 'csrc', f)).read()


def test_module_imports_without_torch_or_the_library():
    code = ("import sys, deep_calcium_amd.merge as m; "
            "assert 'torch' not in sys.modules and 'deep_calcium_amd._lib' not in sys.modules; print(','.join(m.KINDS))")
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == 'moments,corr', out.stderr[-500:]


# ---- neighbours ------------------------------------------------------------------------------------------------------------------
def _box(y0, x0, h, w):
    return np.array([[y, x] for y in range(y0, y0 + h) for x in range(x0, x0 + w)], np.int64)


def test_roi_neighbours_at_distances_0_1_2_on_hand_made_rois():
    from deep_calcium_amd import roi_neighbours
    shape = (12, 24)
    rois = [_box(1, 1, 3, 3),          # 0
            _box(3, 3, 2, 2),          # 1: shares (3, 3) with 0
            _box(1, 4, 2, 2),          # 2: touches 0 side by side (x = 3 | 4), touches 1 at a corner ((2, 5) | (3, 4)): distance 1
            _box(1, 7, 3, 1),          # 3: one blank column (x = 6) between it and 2: distance 2
            _box(1, 10, 3, 1),         # 4: two blank columns after 3: distance 3
            _box(8, 20, 2, 2)]         # 5: far away
    want = {0: [(0, 1)], 1: [(0, 1), (0, 2), (1, 2)], 2: [(0, 1), (0, 2), (1, 2), (2, 3)], 3: [(0, 1), (0, 2), (1, 2), (1, 3), (2, 3), (3, 4)]}
    for d, pairs in want.items():
        got = roi_neighbours(rois, shape, max_dist=d)
        assert got.dtype == np.int32 and got.shape == (len(pairs), 2) and got.tolist() == [list(p) for p in pairs], (d, got.tolist())
        assert ref.neighbours([r.tolist() for r in rois], d) == pairs
    assert roi_neighbours(rois, shape).tolist() == roi_neighbours(rois, shape, max_dist=2).tolist()          # the default
    assert roi_neighbours(rois, shape, max_dist=16).tolist() == ref_pairs(rois, 16)
    # a single ROI, and ROIs that are all apart: no pairs, still (0, 2)
    none = roi_neighbours([rois[0], rois[5]], shape, max_dist=2)
    assert none.shape == (0, 2) and none.dtype == np.int32
    # every form rois_to_csr takes: a labelled mask (its regions are 8-connected, so they never touch: distance 2 is the first), a stack
    mask = np.zeros(shape, np.uint8)
    for r in (rois[0], rois[3], rois[5]):
        mask[r[:, 0], r[:, 1]] = 1
    assert roi_neighbours(mask, shape, max_dist=3).tolist() == [] and roi_neighbours(mask, shape, max_dist=4).tolist() == [[0, 1]]
    stack = np.zeros((3,) + shape, np.uint8)
    for n, r in enumerate((rois[0], rois[1], rois[2])):
        stack[n][r[:, 0], r[:, 1]] = 1
    assert roi_neighbours(stack, shape, max_dist=0).tolist() == [[0, 1]]
    assert roi_neighbours([dict(coordinates=r.tolist()) for r in rois[:3]], shape, max_dist=1).tolist() == [[0, 1], [0, 2], [1, 2]]
    # the image border clips the dilation, nothing wraps around a row end: (0, 23) and (1, 0) are far apart
    assert roi_neighbours([np.array([[0, 23]]), np.array([[1, 0]])], shape, max_dist=2).shape == (0, 2)


def ref_pairs(rois, d):
    return [list(p) for p in ref.neighbours([r.tolist() for r in rois], d)]


def test_roi_neighbours_random_layouts_equal_brute_force():
    from deep_calcium_amd import roi_neighbours
    rs = np.random.RandomState(5)
    shape = (30, 40)
    for trial in range(6):
        rois = []
        for _ in range(12):
            y0, x0 = rs.randint(0, 26), rs.randint(0, 36)
            box = _box(y0, x0, rs.randint(1, 5), rs.randint(1, 5))
            rois.append(box[rs.rand(len(box)) < 0.8] if len(box) > 2 else box)
        rois = [r for r in rois if len(r)]
        for d in (0, 1, 2, 5):
            assert roi_neighbours(rois, shape, max_dist=d).tolist() == ref_pairs(rois, d), (trial, d)


# ---- every ValueError ---------------------------------------------------------------------------------------------------------------
def test_arguments_are_refused_before_the_gpu_is_touched():
    from deep_calcium_amd import TracePairCorr, merge_rois, merge_rois_device, roi_neighbours
    shape = (8, 8)
    rois = [_box(0, 0, 2, 2), _box(0, 3, 2, 2)]
    for bad in (-1, 17, 1.0, True, None, '2'):
        with pytest.raises(ValueError, match='max_dist'):
            roi_neighbours(rois, shape, max_dist=bad)
        with pytest.raises(ValueError, match='max_dist'):
            merge_rois_device('nowhere.npz', rois, max_dist=bad)
    with pytest.raises(ValueError, match='shape'):
        roi_neighbours(rois, (8,))
    with pytest.raises(ValueError, match='outside'):
        roi_neighbours([_box(7, 7, 2, 2)], shape)
    sums = np.arange(3 * 10, dtype=np.int64).reshape(3, 10)
    areas = np.array([4, 4, 4])
    ok = np.array([[0, 1], [1, 2]], np.int32)
    # sums, as dff._check_sums does
    for bad in (sums.astype(np.int32), sums[0], sums.tolist(), np.zeros((0, 5), np.int64), np.zeros((2, 0), np.int64)):
        with pytest.raises(ValueError, match='sums'):
            TracePairCorr(bad, areas, ok)
    for bad in (np.array([4, 4]), np.array([4.0, 4.0, 4.0]), np.array([4, 0, 4]), np.array([[4, 4, 4]])):
        with pytest.raises(ValueError, match='areas'):
            TracePairCorr(sums, bad, ok)
    # pairs
    for bad in (np.array([0, 1, 2]), np.array([[0, 1, 2]]), np.array([[0.0, 1.0]]), np.array([[[0, 1]]]), 'ab', None):
        with pytest.raises(ValueError, match='pairs must be'):
            TracePairCorr(sums, areas, bad)
    for bad, text in (([[0, 3]], r'pair 0 = \(0, 3\)'), ([[0, 1], [-1, 0]], r'pair 1 = \(-1, 0\)'), ([[2 ** 31 - 1, 0]], 'outside')):
        with pytest.raises(ValueError, match=text):
            TracePairCorr(sums, areas, np.array(bad))
    # L
    for bad in (0, 1, 4097, -2, 2.0, True, '128'):
        with pytest.raises(ValueError, match='detrend_frames'):
            TracePairCorr(sums, areas, ok, detrend_frames=bad)
        with pytest.raises(ValueError, match='detrend_frames'):
            merge_rois_device('nowhere.npz', rois, detrend_frames=bad)
    # the range: max(M, T) * max(areas) <= 2**46, naming the ROI.  T = 2**17: M = T; L = 4096: 32 segments, M = 4096 * 4096 = 2**24 > T
    long = np.zeros((3, 1 << 17), np.int64)
    with pytest.raises(ValueError, match=r'ROI 1 has %d pixels.*2\*\*46' % (2 ** 29 + 1)):
        TracePairCorr(long, np.array([4, 2 ** 29 + 1, 4]), ok)
    with pytest.raises(ValueError, match=r'ROI 2 has %d pixels: max\(M, T\) \* area = %d \* ' % (2 ** 22 + 1, 2 ** 24)):
        TracePairCorr(long, np.array([4, 4, 2 ** 22 + 1]), ok, detrend_frames=4096)
    with pytest.raises(ValueError, match='areas'):
        TracePairCorr(sums, np.array([4, 4, 2 ** 30 + 1]), ok)
    # inside the range every argument is accepted up to the GPU: without one, the loud refusal
    import torch
    if not torch.cuda.is_available():
        from deep_calcium_amd._lib import DcunetError
        for areas_ok, L in (([4, 2 ** 29, 4], None), ([4, 4, 2 ** 22], 4096), ([2 ** 29, 4, 4], 2)):
            with pytest.raises(DcunetError, match='no CPU fallback'):
                TracePairCorr(long, np.array(areas_ok), ok, detrend_frames=L)
    # kinds
    from deep_calcium_amd.merge import _check_kind
    with pytest.raises(ValueError, match='kind'):
        _check_kind('gram')
    # merge_rois
    pix = [r for r in rois]
    for bad in (float('nan'), 'x', None, True):
        with pytest.raises(ValueError, match='threshold'):
            merge_rois(pix, [[0, 1]], [0.9], shape, threshold=bad)
        with pytest.raises(ValueError, match='threshold'):
            merge_rois_device('nowhere.npz', rois, threshold=bad)
    for bad in ([float('nan')], ['a'], [None], [[0.9]], [0.9, 0.9], []):
        with pytest.raises(ValueError, match='corr|pairs'):
            merge_rois(pix, [[0, 1]], bad, shape)
    with pytest.raises(ValueError, match='outside'):
        merge_rois(pix, [[0, 2]], [0.9], shape)
    with pytest.raises(ValueError, match='pairs must be'):
        merge_rois(pix, [[0.0, 1.0]], [0.9], shape)
    with pytest.raises(ValueError, match='pixels must be a list'):
        merge_rois(np.zeros(shape, np.uint8), [[0, 1]], [0.9], shape)
    with pytest.raises(ValueError, match='outside the 8 x 8 image'):
        merge_rois([_box(7, 7, 2, 2)], np.zeros((0, 2), np.int32), [], shape)
    with pytest.raises(ValueError, match='not both'):
        merge_rois_device('nowhere.npz', rois, shifts=np.zeros((4, 2), np.int32), fine_shifts=np.zeros((4, 2), np.int32))
    with pytest.raises(ValueError, match='bidi'):
        merge_rois_device('nowhere.npz', rois, bidi=1.5)


# ---- the merge rule ---------------------------------------------------------------------------------------------------------------
def _same(new, origin, want):
    return len(new) == len(want[0]) and all(n.dtype == np.int64 and n.tolist() == [list(p) for p in w] for n, w in zip(new, want[0])) \
        and origin == want[1]


def test_merge_rule_chain_components_ordering_and_duplicates():
    from deep_calcium_amd import merge_rois
    shape = (10, 30)
    W = shape[1]
    rois = [_box(5, 20, 2, 2),         # 0: merges with 5 -- the component's smallest flat index comes from 5
            _box(0, 10, 2, 2),         # 1  chain 1-2-3: 1-2 and 2-3 accepted, 1-3 low
            _box(0, 12, 2, 2),         # 2
            _box(0, 13, 2, 3),         # 3: overlaps 2 in column 13: the union lists those pixels once
            _box(0, 0, 1, 2),          # 4: on no accepted edge: unchanged, first in the output
            _box(3, 18, 2, 2),         # 5
            _box(8, 0, 1, 1)]          # 6: on a rejected edge only
    pairs = [(1, 2), (2, 3), (1, 3), (5, 0), (4, 6), (2, 2), (1, 2)]
    corr = [0.8, 0.95, 0.1, 0.81, 0.7999, -1.0, 0.2]        # 0.8 itself is accepted; a repeated pair below the threshold changes nothing
    new, origin = merge_rois(rois, np.array(pairs), np.array(corr, np.float32), shape, threshold=np.float32(0.8))
    want = ref.merge([r.tolist() for r in rois], pairs, [float(np.float32(c)) for c in corr], W, float(np.float32(0.8)))
    assert _same(new, origin, want)
    assert origin == [[4], [1, 2, 3], [0, 5], [6]]
    chain = new[1]
    assert len(chain) == 4 + 4 + 6 - 2 and len(set(map(tuple, chain.tolist()))) == len(chain)          # the overlap counted once
    flat = chain[:, 0] * W + chain[:, 1]
    assert (np.diff(flat) > 0).all()                                                                    # sorted by flat index
    assert [int(n[0, 0]) * W + int(n[0, 1]) for n in new] == sorted(int(n[0, 0]) * W + int(n[0, 1]) for n in new)
    assert new[0].tolist() == rois[4].tolist() and new[3].tolist() == rois[6].tolist()                  # unchanged
    # single linkage: raising the threshold above the weakest link cuts the chain there
    new, origin = merge_rois(rois, pairs, corr, shape, threshold=0.9)
    assert origin == [[4], [1], [2, 3], [5], [0], [6]]
    # no pairs at all, and pairs that are all rejected: every ROI comes through, ordered by smallest flat index
    for p, c in ((np.zeros((0, 2), np.int32), np.zeros(0, np.float32)), (pairs, [-1.0] * len(pairs))):
        new, origin = merge_rois(rois, p, c, shape)
        assert origin == [[4], [1], [2], [3], [5], [0], [6]] and all(n.tolist() == rois[o[0]].tolist() for n, o in zip(new, origin))
    # unsorted, repeated pixels in the input are sorted and de-duplicated; ROIs that share their smallest pixel keep their order
    a = np.array([[2, 2], [1, 1], [1, 1], [1, 2]])
    b = np.array([[1, 1], [5, 5]])
    new, origin = merge_rois([b, a], [[0, 1]], [0.0], shape)
    assert origin == [[0], [1]] and new[0].tolist() == [[1, 1], [5, 5]] and new[1].tolist() == [[1, 1], [1, 2], [2, 2]]
    new, origin = merge_rois([b, a], [[1, 0]], [1.0], shape)
    assert origin == [[0, 1]] and new[0].tolist() == [[1, 1], [1, 2], [2, 2], [5, 5]]
    # an infinite corr is a number
    assert merge_rois([b, a], [[1, 0]], [float('inf')], shape)[1] == [[0, 1]] and merge_rois([b, a], [[1, 0]], [float('-inf')], shape)[1] == [[0], [1]]


def test_merge_rule_random_graphs_equal_the_flood_fill():
    from deep_calcium_amd import merge_rois
    rs = np.random.RandomState(9)
    shape = (20, 20)
    for trial in range(20):
        R = rs.randint(1, 12)
        rois = [_box(rs.randint(0, 17), rs.randint(0, 17), rs.randint(1, 4), rs.randint(1, 4)) for _ in range(R)]
        P = rs.randint(0, 2 * R + 1)
        pairs = rs.randint(0, R, size=(P, 2))
        corr = rs.uniform(-1, 1, size=P).astype(np.float32)
        new, origin = merge_rois(rois, pairs, corr, shape, threshold=0.2)
        assert _same(new, origin, ref.merge([r.tolist() for r in rois], pairs.tolist(), corr.tolist(), shape[1], 0.2)), trial
        assert sorted(r for o in origin for r in o) == list(range(R))


# ---- the reach of the rule, on the exact oracle ---------------------------------------------------------------------------------------
SEEDS = range(40)


def test_reach_table_bleaching_merges_distinct_cells_and_detrending_parts_them():
    """_pair_ref.scene(kind, seed, 60, 30, T = 1024), seeds 0..39, the left and the right half of the region as two ROIs, threshold
    0.8, quotients of the exact integer numerators.  Undecayed, None: the halves of ONE cell ('same') merge in 40 of 40 scenes,
    the two cells of 'two' in 0.  Decayed to half the brightness, None: 'two' merges in 40 of 40 -- the failure detrending
    fixes.  Decayed, L = 128: 'two' 0 of 40, 'same' 40 of 40."""
    table = {}
    for kind in ('two', 'same'):
        for beta, L in ((None, None), (0.5, None), (0.5, 128)):
            c = [ref.half_corr(kind, seed, L, T=1024, beta=beta) for seed in SEEDS]
            table[kind, beta, L] = c
            print('%-4s decay %-4s L %-4s corr %.3f .. %.3f   merged at 0.8: %d / %d' % (kind, beta, L, min(c), max(c), sum(v >= 0.8 for v in c), len(c)))
    merged = dict((k, sum(v >= 0.8 for v in c)) for k, c in table.items())
    assert merged['same', None, None] == 40 and merged['two', None, None] == 0
    assert merged['two', 0.5, None] == 40
    assert merged['two', 0.5, 128] == 0 and merged['same', 0.5, 128] == 40
    assert merged['same', 0.5, None] == 40
    # and the merge rule on those numbers does what the counts say
    from deep_calcium_amd import merge_rois
    left, right = _box(2, 2, 6, 6), _box(2, 8, 6, 6)
    for (kind, beta, L), c in table.items():
        for v in c[:3]:
            _, origin = merge_rois([left, right], [[0, 1]], [v], (10, 16))
            assert origin == ([[0, 1]] if v >= 0.8 else [[0], [1]])


# ---- the oracle itself ----------------------------------------------------------------------------------------------------------------
def test_oracle_numerators_are_the_float64_correlation_on_small_numbers_and_the_words_round_trip():
    rs = np.random.RandomState(3)
    x, y = rs.randint(-1000, 1000, size=50), rs.randint(-1000, 1000, size=50)
    m = ref.moments([x.tolist(), y.tolist()], [(0, 1), (1, 0), (0, 0), (5, 0)], None)
    assert m[3] == (0, 0, 0) and m[0] == (m[1][2], m[1][1], m[1][0]) and m[2][0] == m[2][1] == m[2][2]
    assert abs(ref.corr64(m)[0] - np.corrcoef(x, y)[0, 1]) < 1e-12
    assert ref.corr(m)[2] == np.float32(1) and ref.corr(m)[3] == np.float32(0)
    # pooled over segments: the mean of each segment taken out first
    L = 8
    parts = ref.plan(50, L)
    assert parts[-1] == (40, 10, 8) and ref.big_m(50, L) == 80 and ref.big_m(50, None) == 50 and ref.plan(50, 26) == [(0, 50, 1)]
    xc, yc = x.astype(np.float64).copy(), y.astype(np.float64).copy()
    for t0, n, _ in parts:
        xc[t0:t0 + n] -= xc[t0:t0 + n].mean()
        yc[t0:t0 + n] -= yc[t0:t0 + n].mean()
    mp = ref.moments([x.tolist(), y.tolist()], [(0, 1)], L)
    assert abs(ref.corr64(mp)[0] - (xc * yc).sum() / np.sqrt((xc * xc).sum() * (yc * yc).sum())) < 1e-12
    for n in (0, 1, -1, 2 ** 64, -2 ** 64, 2 ** 124, -2 ** 124 + 12345, 2 ** 63, -2 ** 63):
        lo, hi = ref.words(n)
        assert -2 ** 63 <= lo < 2 ** 63 and -2 ** 63 <= hi < 2 ** 63 and hi * 2 ** 64 + (lo % 2 ** 64) == n


# ---- the scalar arithmetic of the kernels --------------------------------------------------------------------------------------
def test_trace_pair_math_under_the_host_sanitizers(tmp_path):
    """csrc/trace_pair_math.h compiled into tests/native/trace_pair_math_check.cpp with the address and undefined-behaviour
    sanitizers and run as a program of its own: the segment plan against detrend_plan's words, the per-segment term and the
    pooled numerators against __int128 with both rows at the bound +-floor(2^62 / max(M, T)), and the range predicate."""
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
    exe = str(tmp_path / 'trace_pair_math_check')
    src = os.path.join(ROOT, 'tests', 'native', 'trace_pair_math_check.cpp')
    r = subprocess.run([cxx] + flags + [src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'trace_pair_math_check: ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_the_plan_of_the_header_is_detrend_plan():
    """The three statements of the cut agree: series.detrend_plan, tests/_detrend_ref.plan and the words of the header the kernel follows."""
    from deep_calcium_amd import detrend_plan
    for T, L, want in ((1000, 128, [(s * 128, 128, 232) for s in range(6)] + [(768, 232, 128)]), (5, 2, [(0, 2, 3), (2, 3, 2)]),
                       (257, 129, [(0, 257, 1)]), (1, 2, [(0, 1, 1)]), (64, 4096, [(0, 64, 1)])):
        assert detrend_plan(T, L) == ref.plan(T, L) == want, (T, L)
