"""ROI pixel-pair correlation and the split of merged ROIs without a GPU: the public names and the ABI, the tile list and the
state offsets, the reference's own corr against np.corrcoef, split_rois against the naive restatement of tests/_pair_ref.py, the
scenes' conditions on the float64 oracle, argument validation in front of and inside the library, and csrc/pair_math.h as a
stand-alone program under the host sanitizers."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _pair_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES = ('dc_roi_pair_accumulate', 'dc_roi_pair_corr')


def test_public_names_and_abi():
    import deep_calcium_amd
    from deep_calcium_amd import _build, _gen_tape, _lib, footprints, roi_pairs
    for name in ('RoiPairCorr', 'roi_pair_corr_device', 'split_rois', 'split_rois_device'):
        assert getattr(deep_calcium_amd, name) is getattr(roi_pairs, name) and name in deep_calcium_amd.__all__
    assert _lib.header_abi_version() >= 119 and 'roi_pairs.hip' in _build.SOURCES
    assert '-ffp-contract=off' in _build.FILE_FLAGS['roi_pairs.hip']
    protos = _lib.parse_header()
    tapeable = set(n for n, _ in _gen_tape.prototypes())
    for name in LAUNCHES:
        assert name in protos and name in tapeable, name
    assert [len(protos[n][1]) for n in LAUNCHES] == [16, 10]
    header = open(_lib.HEADER).read()
    assert 'ROI pixel-pair correlation' in header
    for text, value in (('DC_ROI_PAIR_TILE 64', roi_pairs.TILE), ('DC_ROI_PAIR_BATCH 32', roi_pairs.BATCH),
                        ('DC_ROI_PAIR_MAX_AREA 1024', roi_pairs.MAX_AREA), ('DC_ROI_PAIR_MAX_STATE 134217728L', roi_pairs.MAX_STATE)):
        assert '#define ' + text in header and int(text.split()[1].rstrip('L')) == value, text
    assert roi_pairs.MAX_STATE == 2 ** 27 and ref.TILE == roi_pairs.TILE
    assert roi_pairs.KINDS == ('moments', 'corr')
    for f in ('roi_pairs.hip', 'pair_math.h'):
        assert '#pragma clang fp contract(off)' in open(os.path.join(ROOT, 'deep_calcium_amd', 'csrc', f)).read()
    # what the footprint module offered stays what it was
    assert footprints.KINDS == ('moments', 'corr', 'coherence') and footprints.MAX_FRAMES == 2 ** 31 - 1


def test_module_imports_without_torch_or_the_library():
    code = ("import sys, deep_calcium_amd.roi_pairs as m; "
            "assert 'torch' not in sys.modules and 'deep_calcium_amd._lib' not in sys.modules; print(','.join(m.KINDS))")
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == 'moments,corr', out.stderr[-500:]


# ---- bookkeeping -----------------------------------------------------------------------------------------------------------
def test_tile_list_and_state_offsets():
    from deep_calcium_amd.roi_pairs import MAX_AREA, pair_layout
    areas = [1, 63, 64, 65, 130]
    roi_off, goff, tiles, G = pair_layout(areas)
    want = ref.layout(areas)
    assert roi_off.dtype == np.int32 and goff.dtype == np.int64 and tiles.dtype == np.int32 and tiles.shape == (1 + 1 + 1 + 3 + 6, 3)
    assert roi_off.tolist() == want[0] == [0, 1, 64, 128, 193, 323]
    assert goff.tolist() == want[1] == [0, 1, 1 + 63 ** 2, 1 + 63 ** 2 + 64 ** 2, 1 + 63 ** 2 + 64 ** 2 + 65 ** 2]
    assert G == want[3] == sum(k * k for k in areas)
    assert [tuple(t) for t in tiles.tolist()] == want[2]
    assert [tuple(t) for t in tiles.tolist()][3:] == [(3, 0, 0), (3, 0, 1), (3, 1, 1), (4, 0, 0), (4, 0, 1), (4, 0, 2), (4, 1, 1), (4, 1, 2), (4, 2, 2)]
    # every pair i <= j of every ROI lies in exactly one tile
    for r, k in enumerate(areas):
        seen = np.zeros((k, k), int)
        for rr, ti, tj in tiles.tolist():
            if rr == r:
                seen[ti * 64:(ti + 1) * 64, tj * 64:(tj + 1) * 64] += 1
        upper = np.triu(np.ones((k, k), bool))
        assert (seen[upper] == 1).all() and (seen <= 1).all() and (np.tril(seen, -64) == 0).all()
    assert len(pair_layout([MAX_AREA])[2]) == 136
    with pytest.raises(ValueError, match='ROI 2 has 1025 pixels'):
        pair_layout([5, 1024, 1025])
    assert pair_layout([1024] * 128)[3] == 2 ** 27
    with pytest.raises(ValueError, match=r'ROI 128 brings.*2\*\*27'):
        pair_layout([1024] * 128 + [1])
    with pytest.raises(ValueError, match='ROI 1 is empty'):
        pair_layout([3, 0])


# ---- the reference itself --------------------------------------------------------------------------------------------------
def test_reference_corr_is_numpys_corrcoef():
    """Series small enough that float64 is exact: 12 pixels, T = 37."""
    rs = np.random.RandomState(5)
    T, H, W = 37, 5, 7
    frames = rs.randint(-200, 200, size=(T, H, W)).astype(np.int16)
    frames[:, 2, 2:5] += (rs.randint(0, 300, size=T)[:, None]).astype(np.int16)
    flat = [9, 10, 16, 17, 18, 19, 23, 24, 25, 30, 31, 34]
    a, g = ref.moments(frames, flat)
    want = np.corrcoef(frames.reshape(T, -1)[:, flat].astype(np.float64).T)
    plain, exact = ref.matrix(T, a, g, ref.corr64), ref.matrix(T, a, g)
    assert np.abs(plain - want).max() < 1e-12 and np.abs(exact.astype(np.float64) - want).max() < 1e-6
    assert np.array_equal(exact, exact.T) and (np.diag(exact) == 1).all()


# ---- split_rois ----------------------------------------------------------------------------------------------------------------
def _same_split(got, want):
    assert got[1] == want[1] and len(got[0]) == len(want[0])
    for g, w in zip(got[0], want[0]):
        assert g.dtype == np.int64 and np.array_equal(g, w)
    assert got[2].dtype == np.float64 and np.allclose(got[2], want[2], rtol=0, atol=1e-12, equal_nan=True)


def _blocks(groups, inside=0.75, across=0.25):
    groups = np.asarray(groups)
    C = np.where(groups[:, None] == groups[None, :], inside, across)
    np.fill_diagonal(C, 1.0)
    return C


def test_split_rois_on_hand_made_matrices():
    from deep_calcium_amd import split_rois
    shape = (4, 20)
    strip = np.array([[1, x] for x in range(16)])
    # group 1 = pixels 0..4 and the stray pixel 10; group 0 = 5..9 and 11..15: two components of 5, the first wins the tie
    C = _blocks([1] * 5 + [0] * 5 + [1] + [0] * 5)
    new, origin, gaps = split_rois([strip], [C.astype(np.float32)], shape, min_gap=0.1, min_area=4)
    assert origin == [0, 0] and new[0].tolist() == strip[0:5].tolist() and new[1].tolist() == strip[5:10].tolist()
    assert gaps.tolist() == [0.5]                                                       # 0.75 - 0.25, exact
    _same_split((new, origin, gaps), ref.split([strip], [C], shape, min_gap=0.1, min_area=4))
    block = np.array([[y, x] for y in (2, 3) for x in range(3, 11)])                    # 2 x 8: left and right 2 x 4
    B = _blocks([0, 0, 0, 0, 1, 1, 1, 1] * 2)
    ones = np.ones((16, 16))
    small = np.array([[0, 0], [0, 1], [0, 2]])
    rois, mats = [small, block, strip, block, block], [np.eye(3), B, C, ones, None]
    for kw in (dict(min_area=4), dict(min_area=5), dict(min_area=6), dict(min_area=8), dict(min_area=9), dict(min_area=1),
               dict(min_area=4, min_gap=0.5), dict(min_area=4, min_gap=0.5000001), dict(min_area=4, min_gap=-1.0),
               dict(min_area=4, iterations=1), dict(min_area=2, iterations=2)):
        _same_split(split_rois(rois, mats, shape, **kw), ref.split(rois, mats, shape, **kw))
    new, origin, gaps = split_rois(rois, mats, shape, min_area=4)
    assert origin == [0, 1, 1, 2, 2, 3, 4]
    assert new[1].tolist() == [[y, x] for y in (2, 3) for x in range(3, 7)] and new[2].tolist() == [[y, x] for y in (2, 3) for x in range(7, 11)]
    assert np.array_equal(new[0], small) and np.array_equal(new[5], block) and np.array_equal(new[6], block)
    assert np.isnan(gaps[[0, 3, 4]]).all() and gaps[[1, 2]].tolist() == [0.5, 0.5]      # too small; one cluster is empty; no matrix
    new, origin, gaps = split_rois(rois, mats, shape, min_area=6)                        # the strip's parts have 5 pixels: the gap is still reported
    assert origin == [0, 1, 1, 2, 3, 4] and gaps[2] == 0.5
    assert split_rois(rois, mats, shape, min_area=4, min_gap=0.5)[1] == [0, 1, 1, 2, 2, 3, 4]
    assert split_rois(rois, mats, shape, min_area=4, min_gap=0.5000001)[1] == [0, 1, 2, 3, 4]
    # matrices whose entries are multiples of 1/8: sums are exact, the two implementations must agree on every label
    rs = np.random.RandomState(3)
    grid = np.array([[y, x] for y in range(4) for x in range(5)])
    for _ in range(20):
        M = rs.randint(-8, 9, size=(20, 20)) / 8.0
        M = np.triu(M, 1) + np.triu(M, 1).T + np.eye(20)
        for kw in (dict(min_area=2, min_gap=-2.0), dict(min_area=2, min_gap=0.0, iterations=3)):
            _same_split(split_rois([grid], [M], shape, **kw), ref.split([grid], [M], shape, **kw))
    for args, kw, what in ((([strip], [C, C], shape), {}, 'matrices'), (([strip], [C], shape), {'min_area': 0}, 'min_area'),
                           (([strip], [C], shape), {'min_area': 2.0}, 'min_area'), (([strip], [C], shape), {'iterations': 0}, 'iterations'),
                           (([strip], [C], shape), {'min_gap': 'x'}, 'min_gap'), (([strip], [C], shape), {'min_gap': float('nan')}, 'NaN'),
                           (([strip], [C[:5]], shape), {}, 'matrix'), (([strip], [C.astype(int)], shape), {}, 'matrix'),
                           (([strip[::-1]], [C], shape), {}, 'flat-index order'), (([strip], [C], (1, 5)), {}, 'outside'),
                           (([strip.astype(float)], [C], shape), {}, r'\(k,2\)'), (([strip], [C], (5,)), {}, 'shape')):
        with pytest.raises(ValueError, match=what):
            split_rois(*args, **kw)


def _wrong(new, left, right):
    """Pixels of the two parts that are not where they were planted, and pixels of the region in neither part."""
    sets = [set(map(tuple, p.tolist())) for p in new]
    want = [set(map(tuple, left.tolist())), set(map(tuple, right.tolist()))]
    return len(sets[0] - want[0]) + len(sets[1] - want[1]), len((want[0] | want[1]) - (sets[0] | sets[1]))


def test_the_scenes_meet_their_conditions_on_the_reference():
    """np.corrcoef stands in for the device, 40 seeds per scene.  The three controls are never split.  The two-cell scene is
    split, with no pixel misassigned and none dropped, in every seed in which both cells fire at least 5 events (7.7 are expected
    at rate 0.03 over 256 frames; a cell that fires once or not at all in the recording has no variance of its own to correlate
    with and no rule separates it: that is the rule's reach, and a seed below it must still misassign nothing)."""
    from deep_calcium_amd import split_rois
    seen = dict((k, [0, []]) for k in ref.SCENES)
    often = 0
    for seed in range(40):
        for kind in ref.SCENES:
            frames, region, left, right, events = ref.scene(kind, seed)
            C = ref.corrcoef(frames, region)
            new, origin, gaps = split_rois([region], [C], frames.shape[1:], min_gap=0.1, min_area=8, iterations=16)
            seen[kind][0] += len(new) == 2
            seen[kind][1].append(gaps[0])
            if kind != 'two':
                assert len(new) == 1 and np.array_equal(new[0], region) and not gaps[0] >= 0.1, (kind, seed, gaps[0])
                continue
            if len(new) == 2:
                assert _wrong(new, left, right) == (0, 0) and origin == [0, 0] and gaps[0] >= 0.1, seed
            if min(events) >= 5:
                often += 1
                assert len(new) == 2, (seed, events, gaps[0])
            if seed < 4:                                                                # the naive restatement agrees
                _same_split((new, origin, gaps), ref.split([region], [C], frames.shape[1:]))
    for kind in ref.SCENES:
        print('%-6s split %2d of 40, gap min %.3f max %.3f' % (kind, seen[kind][0], np.nanmin(seen[kind][1]), np.nanmax(seen[kind][1])))
    assert often >= 20 and seen['two'][0] >= often


def test_the_gpu_scene_meets_its_conditions_on_the_reference():
    """What tests/test_roi_pairs_gpu.py relies on: on the float64 oracle the planted region is split exactly and with a gap of at
    least 0.15 (min_gap is 0.1: a difference of one float32 ulp in the matrix cannot decide the outcome), every control's gap is
    below 0.05 or undefined, and the strip is too small to be looked at."""
    from deep_calcium_amd import split_rois
    frames, rois, left, right = ref.gpu_scene()
    assert frames.shape == (256, 10, 64) and frames.dtype == np.int16 and [len(r) for r in rois] == [72, 72, 9, 72, 72]
    C = [ref.corrcoef(frames, r) for r in rois]
    for fn in (split_rois, ref.split):
        new, origin, gaps = fn(rois, C, frames.shape[1:], min_gap=0.1, min_area=8, iterations=16)
        assert origin == [0, 1, 1, 2, 3, 4]
        assert np.array_equal(new[1], left) and np.array_equal(new[2], right)
        for n, r in ((0, 0), (3, 2), (4, 3), (5, 4)):
            assert np.array_equal(new[n], rois[r])
        assert gaps[1] >= 0.15 and np.isnan(gaps[2]) and all(not g >= 0.05 for g in gaps[[0, 3, 4]]), gaps


# ---- validation ----------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    from deep_calcium_amd import _lib, roi_pairs

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'lib', boom)
    ok = [np.array([[1, 2], [3, 4]])]
    big = [np.array([[0, 0]]), np.array([[y, x] for y in range(33) for x in range(32)])[:1025]]
    P = roi_pairs.RoiPairCorr
    for args, kw, what in ((((5, 7), 4, np.float32, ok), {}, 'int16 or uint16'),
                           (((5,), 4, np.int16, ok), {}, 'shape'),
                           (((5, 7), 0, np.int16, ok), {}, 'n_frames'),
                           (((5, 7), 2 ** 46 // 35 + 1, np.int16, ok), {}, r'2\*\*46'),
                           (((1, 1), 2 ** 31, np.int16, [np.array([[0, 0]])]), {}, r'2\*\*31 - 1'),
                           (((5, 7), 4, np.int16, []), {}, 'no ROIs'),
                           (((5, 7), 4, np.int16, [np.array([[5, 7]])]), {}, 'outside'),
                           (((33, 32), 4, np.int16, big), {}, 'ROI 1 has 1025 pixels'),
                           (((5, 7), 4, np.int16, ok), {'chunk_frames': 0}, 'chunk_frames'),
                           (((5, 7), 4, np.int16, ok), {'shifts': np.zeros((3, 2), int)}, 'shifts'),
                           (((5, 7), 4, np.int16, ok), {'shifts': np.zeros((4, 2), int), 'fine_shifts': np.zeros((4, 2), int)}, 'not both')):
        with pytest.raises(ValueError, match=what):
            P(*args, **kw)
    whole = [np.array([[y, x] for y in range(32) for x in range(32)])] * 129             # 129 x 1024^2 > 2^27
    with pytest.raises(ValueError, match=r'ROI 128 brings.*2\*\*27'):
        P((32, 32), 4, np.int16, whole)
    for kw, what in ((dict(min_area=0), 'min_area'), (dict(iterations=0), 'iterations'), (dict(min_gap=None), 'min_gap'),
                     (dict(shifts=np.zeros((4, 2), int), fine_shifts=np.zeros((4, 2), int)), 'not both')):
        with pytest.raises(ValueError, match=what):
            roi_pairs.split_rois_device('/nonexistent/dataset.npz', ok, **kw)
    with pytest.raises(ValueError, match='not both'):
        roi_pairs.roi_pair_corr_device('/nonexistent/dataset.npz', ok, shifts=np.zeros((4, 2), int), fine_shifts=np.zeros((4, 2), int))


def test_c_abi_argument_validation_returns_codes(dclib):
    """Refused before any launch (there is no GPU here): the pointers are never followed."""
    from deep_calcium_amd._lib import DcunetError
    p = 4096                                  # any aligned non-null value
    acc, cor = dclib.dc_roi_pair_accumulate, dclib.dc_roi_pair_corr

    def A(frames=p, uns=0, tc=1, off=p, pix=p, goff=p, tiles=p, ntiles=0, R=1, a=p, g=p, P=4, G=16, H=5, W=7):
        return acc(frames, uns, tc, off, pix, goff, tiles, ntiles, R, a, g, P, G, H, W, None)
    for kw in (dict(frames=None), dict(off=None), dict(pix=None), dict(goff=None), dict(tiles=None), dict(a=None), dict(g=None)):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            A(**kw)
    for kw in (dict(tc=-1), dict(ntiles=-1), dict(R=-1), dict(P=-1), dict(G=-1)):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
            A(**kw)
    with pytest.raises(DcunetError, match=r'\(-1\).*out of range'):
        A(H=2 ** 15, W=2 ** 15 + 1)
    for kw in (dict(frames=p + 1), dict(off=p + 2), dict(pix=p + 2), dict(tiles=p + 2), dict(goff=p + 4), dict(a=p + 4), dict(g=p + 4)):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            A(**kw)
    assert A(tc=2 ** 16, H=2 ** 15, W=2 ** 15) == 0                                       # the last chunk that fits (no tiles: nothing launched)
    with pytest.raises(DcunetError, match=r'\(-3\).*2\^46 = 70368744177664'):
        A(tc=2 ** 16 + 1, H=2 ** 15, W=2 ** 15)
    assert A(P=2 ** 17, G=2 ** 27) == 0
    with pytest.raises(DcunetError, match=r'\(-3\).*2\^27 = 134217728'):
        A(P=2 ** 18, G=2 ** 27 + 1)
    assert A(P=4, G=4096) == 0
    with pytest.raises(DcunetError, match=r'\(-3\).*more than 1024 pixels'):
        A(P=4, G=4097)
    with pytest.raises(DcunetError, match=r'\(-3\).*2\^31 - 1'):
        A(ntiles=2 ** 31, R=2 ** 31 - 1)
    with pytest.raises(DcunetError, match=r'\(-3\).*137 tiles for 1 ROIs'):
        A(ntiles=137)
    assert A() == 0 and A(ntiles=1, tc=0) == 0 and A(ntiles=1, P=0, G=0) == 0 and A(ntiles=0, R=0) == 0      # empty work: nothing launched

    def C(a=p, g=p, off=p, goff=p, R=1, P=4, G=16, T=8, corr=p):
        return cor(a, g, off, goff, R, P, G, T, corr, None)
    for kw in (dict(a=None), dict(g=None), dict(off=None), dict(goff=None), dict(corr=None)):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            C(R=0, **kw)
    for kw in (dict(R=-1), dict(P=-1), dict(G=-1), dict(T=-1)):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
            C(**kw)
    for kw in (dict(a=p + 4), dict(g=p + 4), dict(goff=p + 4), dict(off=p + 2), dict(corr=p + 2)):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            C(R=0, **kw)
    assert C(R=0, T=2 ** 31 - 1) == 0
    with pytest.raises(DcunetError, match=r'\(-3\).*2\^31 - 1'):
        C(R=0, T=2 ** 31)
    with pytest.raises(DcunetError, match=r'\(-3\).*2\^27 = 134217728'):
        C(R=0, P=2 ** 18, G=2 ** 27 + 1)
    with pytest.raises(DcunetError, match=r'\(-3\).*more than 1024 pixels'):
        C(R=0, P=4, G=4097)
    assert C(R=0) == 0 and C(P=0, G=0) == 0


# ---- the scalar arithmetic of the kernels --------------------------------------------------------------------------------------
def test_pair_math_under_the_host_sanitizers(tmp_path):
    """csrc/pair_math.h compiled into tests/native/pair_math_check.cpp with the address and undefined-behaviour sanitizers and
    run as a program of its own: the numerators against __int128 at the limits, the symmetry, the diagonal and the edge cases of
    the correlation, the tile count and the range check of an ROI."""
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
    exe = str(tmp_path / 'pair_math_check')
    src = os.path.join(ROOT, 'tests', 'native', 'pair_math_check.cpp')
    r = subprocess.run([cxx] + flags + [src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'pair_math_check: ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_frames_of_one_call_are_limited(dclib):
    """DC_FRAMES_PER_CALL_MAX: tc = 2^30 + 1 is refused with (-3) and the limit's message before any launch, tc = 2^30 is not."""
    import _wideindex
    _wideindex.check_frame_limit(dclib, 'test_roi_pairs_api')
