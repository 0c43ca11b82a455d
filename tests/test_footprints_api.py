"""ROI footprint maps without a GPU: the public names and the ABI, roi_support and refine_rois against the naive restatements of
tests/_footprints_ref.py, the reference's own corr against np.corrcoef, the synthetic scene's conditions on the reference, argument
validation in front of and inside the library, and csrc/footprint_math.h as a stand-alone program under the host sanitizers."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _footprints_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES = ('dc_roi_pixel_accumulate', 'dc_roi_trace_moments', 'dc_roi_pixel_corr')


def test_public_names_and_abi():
    import deep_calcium_amd
    from deep_calcium_amd import _build, _gen_tape, _lib, footprints, traces
    for name in ('RoiFootprints', 'roi_footprints_device', 'roi_support', 'refine_rois'):
        assert getattr(deep_calcium_amd, name) is getattr(footprints, name) and name in deep_calcium_amd.__all__
    assert _lib.header_abi_version() >= 117 and 'footprints.hip' in _build.SOURCES
    assert '-ffp-contract=off' in _build.FILE_FLAGS['footprints.hip']
    protos = _lib.parse_header()
    tapeable = set(n for n, _ in _gen_tape.prototypes())
    for name in LAUNCHES:
        assert name in protos and name in tapeable, name
    assert [len(protos[n][1]) for n in LAUNCHES] == [16, 6, 11]
    header = open(_lib.HEADER).read()
    assert 'ROI footprint maps' in header
    assert 'DC_ROI_PIXEL_MAX_FRAMES 2147483647' in header and footprints.MAX_FRAMES == 2147483647 == 2 ** 31 - 1
    assert footprints.KINDS == ('moments', 'corr', 'coherence') and footprints.MAX_HALO == 16
    assert 'DC_FP_MAX_FRAMES 2147483647L' in open(os.path.join(ROOT, 'deep_calcium_amd', 'csrc', 'footprint_math.h')).read()
    for f in ('footprints.hip', 'footprint_math.h'):
        assert '#pragma clang fp contract(off)' in open(os.path.join(ROOT, 'deep_calcium_amd', 'csrc', f)).read()
    # what the traces module offered stays what it was
    assert traces.KINDS == ('sum', 'mean', 'zscore') and traces.SEGMENT_PIXELS == 512


def test_footprints_module_imports_without_torch_or_the_library():
    code = ("import sys, deep_calcium_amd.footprints as f; "
            "assert 'torch' not in sys.modules and 'deep_calcium_amd._lib' not in sys.modules; print(','.join(f.KINDS))")
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == 'moments,corr,coherence', out.stderr[-500:]


# ---- roi_support -----------------------------------------------------------------------------------------------------------
def _rois_for(H, W):
    """ROIs at the corners and edges, two that overlap, one in the middle, a single pixel."""
    rois = [np.array([[0, 0]]), np.array([[H - 1, W - 1]])]
    if H * W > 1:
        rois.append(np.array([[0, W - 1], [min(1, H - 1), W - 1]]))                       # top right corner, along the edge
        rois.append(np.array([[H - 1, 0], [H - 1, min(1, W - 1)], [H - 1, min(2, W - 1)]]))
        cy, cx = H // 2, W // 2
        blob = np.array([[y, x] for y in range(max(0, cy - 1), min(H, cy + 2)) for x in range(max(0, cx - 2), min(W, cx + 2))])
        rois += [blob, blob[len(blob) // 2:], np.concatenate([blob[:3], np.array([[0, cx]])])]      # overlapping; two far parts
    return rois


@pytest.mark.parametrize('shape', [(1, 1), (5, 7), (33, 19)], ids=['1x1', '5x7', '33x19'])
def test_support_equals_the_naive_support(shape):
    from deep_calcium_amd import roi_support
    H, W = shape
    rois = _rois_for(H, W)
    for halo in (0, 1, 3, 16):
        want_c, want_i = ref.support(rois, shape, halo)
        got_c, got_i = roi_support(rois, shape, halo)
        assert len(got_c) == len(got_i) == len(rois)
        for r in range(len(rois)):
            assert got_c[r].dtype == np.int64 and got_i[r].dtype == np.bool_
            assert np.array_equal(got_c[r], want_c[r]) and np.array_equal(got_i[r], want_i[r]), (halo, r)
            flat = got_c[r][:, 0] * W + got_c[r][:, 1]
            assert (np.diff(flat) > 0).all()                                             # sorted, de-duplicated
            assert int(got_i[r].sum()) == len(set(map(tuple, rois[r].tolist())))
        if halo == 0:
            assert all(i.all() for i in got_i)


def test_support_takes_every_input_form():
    from deep_calcium_amd import roi_support
    from deep_calcium_amd.nf_metrics import mask_to_regions
    H, W = 33, 19
    mask = np.zeros((H, W), np.uint8)
    mask[0:3, 0:4] = 1
    mask[10:14, 15:19] = 1
    mask[32, 9] = 1
    regions = mask_to_regions(mask)
    stack = np.zeros((3, H, W), np.int8)
    for i, g in enumerate(regions):
        stack[i, g[:, 0], g[:, 1]] = 1
    rs = np.random.RandomState(0)
    twice = [np.concatenate([g, g[:2]]) for g in regions]                                # any order, up to two pixels twice
    shuffled = [t[rs.permutation(len(t))] for t in twice]
    dicts = [{'coordinates': [[int(y), int(x)] for y, x in g]} for g in regions]
    want = ref.support(regions, (H, W), 2)
    for form in (mask, stack, shuffled, dicts, tuple(regions)):
        got = roi_support(form, (H, W), 2)
        for r in range(3):
            assert np.array_equal(got[0][r], want[0][r]) and np.array_equal(got[1][r], want[1][r])


# ---- refine_rois -----------------------------------------------------------------------------------------------------------
def test_refine_rois_on_hand_made_maps():
    from deep_calcium_amd import refine_rois
    shape = (6, 9)
    row = lambda y, xs: [[y, x] for x in xs]                                              # noqa: E731
    # ROI 0: two components of 3 pixels each above the threshold (a tie): the one with the smallest flat index wins
    c0 = np.array(row(1, range(0, 9)))
    v0 = np.array([0.9, 0.5, 0.3, 0.1, 0.29999, 0.3, 0.7, 0.30000001, 0.0], np.float32)
    # ROI 1: the later component is the larger; (3,3) and (4,4) hold together diagonally
    c1 = np.array(row(3, [0, 1]) + row(3, [3]) + row(4, [4, 5]) + row(5, [8]))
    v1 = np.array([0.5, 0.5, 0.4, 0.4, 0.4, 1.0], np.float32)
    # ROI 2: nothing reaches the threshold; ROI 3: one pixel does
    c2, v2 = np.array(row(0, [0, 1, 2])), np.array([0.2, -1.0, 0.0], np.float32)
    c3, v3 = np.array(row(5, [0, 1, 2])), np.array([0.2, 0.3, 0.0], np.float32)
    coords, corr = [c0, c1, c2, c3], [v0, v1, v2, v3]
    thr = float(np.float32(0.3))                                                          # hit exactly by v0[2], v0[5], v3[1]
    new, kept = refine_rois(coords, corr, shape, threshold=thr)
    assert kept == [0, 1, 3]
    assert new[0].tolist() == row(1, [0, 1, 2]) and new[1].tolist() == row(3, [3]) + row(4, [4, 5]) and new[2].tolist() == row(5, [1])
    assert all(n.dtype == np.int64 for n in new)
    for kw in (dict(threshold=thr), dict(threshold=thr, min_area=2), dict(threshold=thr, min_area=3), dict(threshold=thr, min_area=4),
               dict(threshold=0.45), dict(threshold=-1.0), dict(threshold=1.0), dict(threshold=1.5)):
        got, want = refine_rois(coords, corr, shape, **kw), ref.refine(coords, corr, shape, **kw)
        assert got[1] == want[1] and len(got[0]) == len(want[0]), kw
        for g, w in zip(got[0], want[0]):
            assert np.array_equal(g, w), kw
    assert refine_rois(coords, corr, shape, threshold=thr, min_area=4) == ([], [])       # everything dropped
    assert refine_rois(coords, corr, shape, threshold=thr, min_area=2)[1] == [0, 1]
    assert refine_rois(coords, corr, shape, threshold=1.0)[1] == [1]
    for args, kw, what in (((coords, corr[:3], shape), {}, 'maps'), ((coords, corr, shape), {'min_area': 0}, 'min_area'),
                           ((coords, corr, shape), {'threshold': 'x'}, 'threshold'), ((coords, corr, shape), {'threshold': float('nan')}, 'NaN'),
                           (([c0], [v0[:4]], shape), {}, r'\(k,2\)'), (([c0], [v0], (1, 5)), {}, 'outside'),
                           (([c0], [v0], (5,)), {}, 'shape')):
        with pytest.raises(ValueError, match=what):
            refine_rois(*args, **kw)


# ---- the reference itself --------------------------------------------------------------------------------------------------
def test_reference_corr_is_numpys_corrcoef():
    """Series small enough that float64 is exact: (5, 7), T = 37."""
    rs = np.random.RandomState(5)
    T, H, W = 37, 5, 7
    frames = rs.randint(-200, 200, size=(T, H, W)).astype(np.int16)
    frames[:, 2, 2:5] += (rs.randint(0, 300, size=T)[:, None]).astype(np.int16)
    own = [np.array([[2, 2], [2, 3], [2, 4], [3, 3]]), np.array([[0, 0], [0, 1]])]
    coords, inside = ref.support(own, (H, W), 1)
    seen = {True: 0, False: 0}
    for (mom, corr, exact), c, ins, o in zip(ref.maps(frames, coords, inside, own), coords, inside, own):
        S = frames[:, o[:, 0], o[:, 1]].astype(np.float64).sum(1)
        for k, ((y, x), i) in enumerate(zip(c, ins)):
            xs = frames[:, y, x].astype(np.float64)
            want = np.corrcoef(xs, S - xs if i else S)[0, 1]
            a, b, cc = mom[k]
            u, w = int(S.sum()), int((S * S).sum())
            assert abs(ref.corr64(T, a, b, cc, u, w, bool(i)) - want) < 1e-12
            assert abs(float(corr[k]) - want) < 1e-6 and abs(float(exact[k]) - want) < 1e-6
            seen[bool(i)] += 1
    assert seen[True] == 6 and seen[False] > 10


def test_the_scene_meets_its_conditions_on_the_reference():
    from deep_calcium_amd import refine_rois
    frames, rois, cell, blob = ref.scene()
    H, W = frames.shape[1:]
    coords, inside = ref.support(rois, (H, W), 2)
    m = ref.maps(frames, coords, inside, rois)
    corr = [x[1] for x in m]
    cell_set, blob_set = set(map(tuple, cell.tolist())), set(map(tuple, blob.tolist()))
    true = np.array([tuple(p) in cell_set for p in coords[0].tolist()])
    assert true.sum() == len(cell) and corr[0][true].min() > 0.5
    assert np.abs(corr[0][~true]).max() < 0.2 and np.abs(corr[1]).max() < 0.2            # the ring, the halo, the whole blob
    print('scene: cell min %.3f, elsewhere max |corr| %.3f, blob max |corr| %.3f' %
          (corr[0][true].min(), np.abs(corr[0][~true]).max(), np.abs(corr[1]).max()))
    assert corr[1][inside[1]].astype(np.float64).mean() < 0.1                             # coherence of the blob
    assert len(blob_set) > 10
    for fn in (ref.refine, refine_rois):
        new, kept = fn(coords, corr, (H, W), threshold=0.3)
        assert kept == [0] and np.array_equal(new[0], cell)


# ---- validation ----------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    from deep_calcium_amd import _lib, footprints
    from deep_calcium_amd import roi_support

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'lib', boom)
    ok = [np.array([[1, 2], [3, 4]])]
    F = footprints.RoiFootprints
    for args, kw, what in ((((5, 7), 4, np.float32, ok), {}, 'int16 or uint16'),
                           (((5,), 4, np.int16, ok), {}, 'shape'),
                           (((5, 7), 0, np.int16, ok), {}, 'n_frames'),
                           (((5, 7), 2 ** 46 // 35 + 1, np.int16, ok), {}, r'2\*\*46'),
                           (((1, 1), 2 ** 31, np.int16, [np.array([[0, 0]])]), {}, r'2\*\*31 - 1'),
                           (((5, 7), 4, np.int16, []), {}, 'no ROIs'),
                           (((5, 7), 4, np.int16, [np.array([[5, 7]])]), {}, 'outside'),
                           (((5, 7), 4, np.int16, ok), {'halo': -1}, 'halo'),
                           (((5, 7), 4, np.int16, ok), {'halo': 17}, 'halo'),
                           (((5, 7), 4, np.int16, ok), {'halo': 1.5}, 'halo'),
                           (((5, 7), 4, np.int16, ok), {'chunk_frames': 0}, 'chunk_frames'),
                           (((5, 7), 4, np.int16, ok), {'shifts': np.zeros((3, 2), int)}, 'shifts'),
                           (((5, 7), 4, np.int16, ok), {'shifts': np.zeros((4, 2), int), 'fine_shifts': np.zeros((4, 2), int)}, 'not both')):
        with pytest.raises(ValueError, match=what):
            F(*args, **kw)
    for halo in (-1, 17, 2.0, True):
        with pytest.raises(ValueError, match='halo'):
            roi_support(ok, (5, 7), halo)
        with pytest.raises(ValueError, match='halo'):
            footprints.roi_footprints_device('/nonexistent/dataset.npz', ok, halo=halo)
    with pytest.raises(ValueError, match='outside'):
        roi_support([np.array([[5, 0]])], (5, 7), 1)


def test_c_abi_argument_validation_returns_codes(dclib):
    """Refused before any launch (there is no GPU here): the pointers are never followed."""
    from deep_calcium_amd._lib import DcunetError
    p = 4096                                  # any aligned non-null value
    acc, mo, cor = dclib.dc_roi_pixel_accumulate, dclib.dc_roi_trace_moments, dclib.dc_roi_pixel_corr

    def A(frames=p, uns=0, tc=1, t0=0, off=p, pix=p, roi=p, S=1, R=1, sums=p, ld=8, mom=p, N=4, H=5, W=7):
        return acc(frames, uns, tc, t0, off, pix, roi, S, R, sums, ld, mom, N, H, W, None)
    for kw in (dict(frames=None), dict(off=None), dict(pix=None), dict(sums=None), dict(mom=None)):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            A(**kw)
    for kw in (dict(S=-1), dict(R=-1), dict(N=-1), dict(tc=-1), dict(t0=-1)):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
            A(**kw)
    with pytest.raises(DcunetError, match=r'\(-1\).*ld = 7 is below t0 \+ tc = 8'):
        A(tc=3, t0=5, ld=7)
    with pytest.raises(DcunetError, match=r'\(-1\).*S = 2 and R = 3'):
        A(roi=None, S=2, R=3)
    with pytest.raises(DcunetError, match=r'\(-1\).*out of range'):
        A(H=2 ** 15, W=2 ** 15 + 1)
    for kw in (dict(frames=p + 1), dict(off=p + 2), dict(pix=p + 2), dict(roi=p + 2), dict(sums=p + 4), dict(mom=p + 4)):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            A(**kw)
    # the two limits: the last frame that fits is accepted by the checks (and N == 0 launches nothing)
    T = 2 ** 16                                 # of 2^15 x 2^15 frames
    assert A(t0=T - 1, ld=T, N=0, H=2 ** 15, W=2 ** 15) == 0
    with pytest.raises(DcunetError, match=r'\(-3\).*2\^46 = 70368744177664'):
        A(t0=T, ld=T + 1, N=0, H=2 ** 15, W=2 ** 15)
    assert A(t0=2 ** 31 - 2, ld=2 ** 31, N=0, H=1, W=1) == 0
    with pytest.raises(DcunetError, match=r'\(-3\).*2\^31 - 1 = 2147483647'):
        A(t0=2 ** 31 - 1, ld=2 ** 31, N=0, H=1, W=1)
    assert A(N=0) == 0 and A(tc=0) == 0 and A(R=0) == 0 and A(S=0) == 0                  # empty work: nothing launched

    with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
        mo(None, 8, 1, 8, p, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
        mo(p, 8, 1, 8, None, None)
    for R, T in ((-1, 8), (1, -1)):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
            mo(p, 8, R, T, p, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*ld = 7 is below T = 8'):
        mo(p, 7, 1, 8, p, None)
    for args in ((p + 4, 8, 1, 8, p, None), (p, 8, 1, 8, p + 4, None)):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            mo(*args)
    with pytest.raises(DcunetError, match=r'\(-3\).*2\^31 - 1'):
        mo(p, 2 ** 31, 1, 2 ** 31, p, None)
    assert mo(p, 8, 0, 8, p, None) == 0

    def C(mom=p, N=4, off=p, roi=p, S=1, R=1, inside=p, rmom=p, T=8, corr=p):
        return cor(mom, N, off, roi, S, R, inside, rmom, T, corr, None)
    for kw in (dict(mom=None), dict(off=None), dict(inside=None), dict(rmom=None), dict(corr=None)):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            C(**kw)
    for kw in (dict(N=-1), dict(S=-1), dict(R=-1), dict(T=-1)):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
            C(**kw)
    with pytest.raises(DcunetError, match=r'\(-1\).*S = 2 and R = 3'):
        C(roi=None, S=2, R=3)
    for kw in (dict(mom=p + 4), dict(rmom=p + 4), dict(off=p + 2), dict(roi=p + 2), dict(inside=p + 2), dict(corr=p + 2)):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            C(**kw)
    with pytest.raises(DcunetError, match=r'\(-3\).*2\^31 - 1'):
        C(T=2 ** 31)
    assert C(N=0) == 0 and C(S=0) == 0


# ---- the scalar arithmetic of the kernels --------------------------------------------------------------------------------------
def test_footprint_math_under_the_host_sanitizers(tmp_path):
    """csrc/footprint_math.h compiled into tests/native/footprint_math_check.cpp with the address and undefined-behaviour
    sanitizers and run as a program of its own: the split and the fold, the numerators against __int128 at the limits, the edge
    cases of the correlation."""
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
    exe = str(tmp_path / 'footprint_math_check')
    src = os.path.join(ROOT, 'tests', 'native', 'footprint_math_check.cpp')
    r = subprocess.run([cxx] + flags + [src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'footprint_math_check: ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])


def test_frames_of_one_call_are_limited(dclib):
    """DC_FRAMES_PER_CALL_MAX: tc = 2^30 + 1 is refused with (-3) and the limit's message before any launch, tc = 2^30 is not."""
    import _wideindex
    _wideindex.check_frame_limit(dclib, 'test_footprints_api')
