"""Weighted ROI traces on the device: dc_roi_wtrace_accumulate, WeightedTraceExtractor, and the unchanged downstream kernels on its
sums.  Every comparison of sums is EQUALITY of int64 with the Python-integer oracle of tests/_weighted_ref.py; every output buffer
is pre-filled with a sentinel and the columns outside [t0, t0 + tc) must keep it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _bidi_ref as biref             # noqa: E402
import _dff_ref as dref               # noqa: E402
import _gridcaps as gc                # noqa: E402
import _merge_ref as mref             # noqa: E402
import _motion_ref as moref           # noqa: E402
import _weighted_ref as ref           # noqa: E402

GARBAGE = -0x0123456789abcdef


def _st():
    return torch.cuda.current_stream().cuda_stream


def _odd(a, dtype=np.int16):
    """A 16-bit numpy array on the device, its first element at an ODD element offset of the allocation (2-byte aligned only)."""
    a = np.ascontiguousarray(a).view(dtype).reshape(-1)
    buf = torch.empty(a.size + 1, dtype=torch.int16, device='cuda')
    buf[1:] = torch.from_numpy(a)
    view = buf[1:]
    assert view.data_ptr() % 4 == 2
    return buf, view


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32))).cuda()


def _uns(dtype):
    return int(np.dtype(dtype) == np.dtype(np.uint16))


def _launch(dclib, frames, off, pix, wgt, roi, R, t0=3, pad=5, twice=True):
    """-> (R, tc) int64 sums of the chunk `frames` (tc, H, W), launched at column t0 of a matrix of stride t0 + tc + pad; frames and
    row_wgt at odd element offsets; the columns outside [t0, t0 + tc) keep the sentinel; a second launch gives the same bytes."""
    tc, H, W = frames.shape
    S, ld = len(off) - 1, t0 + tc + pad
    fbuf, f = _odd(frames)
    wbuf, w = _odd(np.asarray(wgt).astype(np.uint16))
    d_off, d_pix, d_roi = _i32(off), _i32(pix), (_i32(roi) if roi is not None else None)
    outs = []
    for run in range(2 if twice else 1):
        sums = torch.full((R, ld), GARBAGE, dtype=torch.int64, device='cuda')
        dclib.dc_roi_wtrace_accumulate(f.data_ptr(), _uns(frames.dtype), tc, t0, d_off.data_ptr(), d_pix.data_ptr(), w.data_ptr(),
                                       d_roi.data_ptr() if roi is not None else None, S, R, sums.data_ptr(), ld, H, W, _st())
        torch.cuda.synchronize()
        outs.append(sums.cpu().numpy())
    got = outs[0]
    assert (got[:, :t0] == GARBAGE).all() and (got[:, t0 + tc:] == GARBAGE).all(), 'a column outside [t0, t0 + tc) was written'
    if twice:
        assert outs[0].tobytes() == outs[1].tobytes()
    return got[:, t0:t0 + tc]


def _frames(rs, shape, dtype):
    info = np.iinfo(dtype)
    f = rs.randint(info.min, info.max + 1, size=shape).astype(dtype)
    f.flat[0], f.flat[-1] = info.min, info.max
    return f


def _check(dclib, frames, off, pix, wgt, roi, R, tag=''):
    got = _launch(dclib, frames, off, pix, wgt, roi, R)
    want = np.array(ref.csr_sums(frames, off, pix, wgt, roi, R), np.int64).reshape(R, frames.shape[0])
    assert got.dtype == np.int64 and np.array_equal(got, want), tag


# ---- 1. the entry point ----------------------------------------------------------------------------------------------------------
def _small_csr(rs, HW):
    """Five CSR rows over an image of HW pixels: two ROIs that overlap with different weights on the shared pixels, zero weights, an
    index below 0 and one beyond the image, a duplicate index with two weights, an empty row.  -> off, pix, wgt."""
    a = rs.permutation(HW)[:17]
    b = np.concatenate([a[:6], rs.permutation(HW)[:9]])                     # shares at least a[:6] with the first row
    c = np.array([0, HW - 1, -1, HW, HW + 5, -2 ** 31, 2 ** 31 - 1, 0])      # both ends, five indices outside, pixel 0 twice
    d = np.zeros(0, np.int64)
    e = rs.permutation(HW)[:5]
    rows = [a, b, c, d, e]
    wgt = [rs.randint(0, 65536, len(r)) for r in rows]
    wgt[0][:3] = [0, 65535, 1]
    wgt[1][:6] = [65535, 0, 7, 256, 1, 300]
    wgt[4][:] = 0                                                            # a row of zero weights
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    return off, np.concatenate(rows), np.concatenate(wgt)


@pytest.mark.parametrize('dtype', [np.int16, np.uint16], ids=['int16', 'uint16'])
@pytest.mark.parametrize('shape', [(7, 9), (10, 16)], ids=['7x9', '10x16'])
def test_sums_equal_the_oracle_on_small_odd_shapes(dclib, shape, dtype):
    H, W = shape
    rs = np.random.RandomState(100 + H + _uns(dtype))
    off, pix, wgt = _small_csr(rs, H * W)
    for tc in (1, 31, 32, 33, 70):
        frames = _frames(rs, (tc, H, W), dtype)
        _check(dclib, frames, off, pix, wgt, None, 5, 'stores, tc %d' % tc)
        # rows 0 and 2 feed ROI 1, row 1 ROI 0, row 3 (empty) ROI 2, row 4 names no ROI; ROI 3 gets no row and must be zeroed
        for roi in ([1, 0, 1, 2, 7], [1, 0, 1, 2, -1]):
            _check(dclib, frames, off, pix, wgt, roi, 4, 'atomics, tc %d' % tc)


def test_no_32_bit_partial_anywhere(dclib):
    """An ROI of 2100 entries (a 10 x 16 image: every pixel many times) with every weight 65535 over pixels all 65535 and all -32768:
    one term is already beyond int32, a lane's share of a piece beyond 2^36.  As one row through row_roi == NULL, and cut into rows of
    512 through the atomics."""
    H, W, n, T = 10, 16, 2100, 3
    rs = np.random.RandomState(7)
    pix = rs.randint(0, H * W, n)
    wgt = np.full(n, 65535)
    cuts = list(range(0, n, 512)) + [n]
    for dtype, value in ((np.uint16, 65535), (np.int16, -32768)):
        frames = np.full((T, H, W), value, dtype)
        for off, roi in (([0, n], None), (cuts, [0] * (len(cuts) - 1))):
            got = _launch(dclib, frames, off, pix, wgt, roi, 1)
            assert got.tolist() == [[n * 65535 * value] * T] == ref.csr_sums(frames, off, pix, wgt, roi, 1), (dtype, roi)
    assert n * 65535 * 65535 > 2 ** 43 and 32 * 65535 * 65535 > 2 ** 36


def test_row_lengths_around_the_wave_and_the_staged_piece(dclib):
    """Rows of 1, 63, 64, 65, 2047, 2048, 2049 entries and an empty one: a wave is 64 lanes, 2048 entries are staged at a time."""
    H, W, tc = 33, 19, 5
    rs = np.random.RandomState(21)
    lengths = [1, 63, 64, 65, 0, 2047, 2048, 2049]
    off = np.concatenate([[0], np.cumsum(lengths)])
    pix = rs.randint(0, H * W, off[-1])
    wgt = rs.randint(0, 65536, off[-1])
    for dtype in (np.int16, np.uint16):
        frames = _frames(rs, (tc, H, W), dtype)
        _check(dclib, frames, off, pix, wgt, None, 8, 'stores')
        _check(dclib, frames, off, pix, wgt, [0, 1, 0, 1, 2, 3, 2, 3], 4, 'atomics')


# ---- 2. past the caps of the launch ------------------------------------------------------------------------------------------------
CAP_SHAPE = (2, 2)
# (row_off, row_pix, row_wgt, row_roi, R): every CSR row an ROI (plain stores); three rows that feed two ROIs (atomics)
CAP_CSR = {'stores': ([0, 3, 5], [0, 1, 3, 2, 3], [65535, 1, 256, 0, 40000], None, 2),
           'atomics': ([0, 2, 3, 5], [0, 1, 2, 3, 0], [3, 65535, 256, 9, 1], [0, 1, 0], 2)}


@pytest.mark.parametrize('form,dtype', [('stores', np.uint16), ('atomics', np.int16)])
def test_sums_of_tiles_beyond_the_grid(dclib, form, dtype):
    """65535 tiles of 32 frames and three more on a 2 x 2 image: the tile dimension of the grid is capped at 65535 and a workgroup
    strides over the rest; with row_roi the zero kernel clears more than 1024 x 256 values.  The recording is periodic
    (tests/_gridcaps.py): the oracle is evaluated on 37 frames and indexed, on the device."""
    (H, W), tc, t0, pad = CAP_SHAPE, gc.TRACE_FRAMES, 3, 5
    off, pix, wgt, roi, R = CAP_CSR[form]
    assert -(-tc // gc.TRACE_TILE) > gc.FRAME_CAP and (roi is None or R * tc > gc.ZERO_CAP)
    rs = np.random.RandomState(900)
    base = gc.base_frames(rs, (H, W), dtype)
    idx = torch.from_numpy(gc.rows(tc)).cuda()
    frames = torch.from_numpy(base.view(np.int16)).cuda()[idx].contiguous()
    ld = t0 + tc + pad
    sums = torch.full((R, ld), GARBAGE, dtype=torch.int64, device='cuda')
    d_off, d_pix, d_roi = _i32(off), _i32(pix), (_i32(roi) if roi is not None else None)
    d_wgt = torch.from_numpy(np.array(wgt, np.uint16).view(np.int16)).cuda()
    dclib.dc_roi_wtrace_accumulate(frames.data_ptr(), _uns(dtype), tc, t0, d_off.data_ptr(), d_pix.data_ptr(), d_wgt.data_ptr(),
                                   d_roi.data_ptr() if roi is not None else None, len(off) - 1, R, sums.data_ptr(), ld, H, W, _st())
    torch.cuda.synchronize()
    assert bool((sums[:, :t0] == GARBAGE).all()) and bool((sums[:, t0 + tc:] == GARBAGE).all()), 'a guard column was written'
    want = torch.from_numpy(np.array(ref.csr_sums(base, off, pix, wgt, roi, R), np.int64)).cuda()      # (R, K)
    assert bool(torch.equal(sums[:, t0:t0 + tc], want[:, idx]))
    del frames, sums
    torch.cuda.empty_cache()


# ---- 3. the extractor --------------------------------------------------------------------------------------------------------------
def _recording(dtype=np.int16):
    """70 frames of 24 x 30, three ROIs: one of 600 pixels (cut into two CSR rows), two small ones that overlap it and each other;
    weights over the whole range, given in a shuffled order."""
    rs = np.random.RandomState(31)
    T, H, W = 70, 24, 30
    frames = _frames(rs, (T, H, W), dtype)
    flat = [rs.permutation(H * W)[:600], np.arange(40, 75), np.arange(60, 110)]
    rois = [np.stack(np.divmod(rs.permutation(f), W), 1) for f in flat]
    weights = [rs.randint(0, 65536, len(c)) for c in rois]
    weights[1][:4] = [0, 65535, 1, 256]
    return frames, rois, weights


def test_extractor_gives_the_same_sums_for_every_chunking():
    from deep_calcium_amd import WeightedTraceExtractor
    frames, rois, weights = _recording()
    T, H, W = frames.shape
    want = ref.roi_sums(frames, rois, weights)
    for plan in ([1] * T, [7] * 10, [32, 32, 6], [70], [3, 29, 1, 37]):
        ext = WeightedTraceExtractor((H, W), T, frames.dtype, rois, weights, chunk_frames=max(plan))
        a = 0
        for n in plan:
            ext.feed(frames[a:a + n])
            a += n
        assert np.array_equal(ext.result('sum'), want), plan
    assert ext.weight_sums_host().tolist() == ref.weight_sums(weights) == ext.areas_host().tolist()
    assert ext.weight_sums_host().dtype == np.int64 and ext.areas_host().dtype == np.int32 and ext.pixel_counts.tolist() == [600, 35, 50]
    # a recording that is already resident, unsigned this time, fed in two pieces
    uframes, _, _ = _recording(np.uint16)
    ext = WeightedTraceExtractor((H, W), T, np.uint16, rois, weights)
    dev = torch.from_numpy(uframes.view(np.int16)).cuda()
    ext.feed(dev[:33]).feed(dev[33:])
    assert ext._stage is None and np.array_equal(ext.sums_device().cpu().numpy(), ref.roi_sums(uframes, rois, weights))
    # region dicts
    ext = WeightedTraceExtractor((H, W), T, frames.dtype, [dict(coordinates=c.tolist()) for c in rois], weights).feed(frames)
    assert np.array_equal(ext.result('sum'), want)


def test_extractor_with_shifts_and_bidi_sums_the_moved_frames():
    from deep_calcium_amd import WeightedTraceExtractor
    frames, rois, weights = _recording()
    T, H, W = frames.shape
    rs = np.random.RandomState(5)
    shifts = rs.randint(-4, 5, size=(T, 2)).astype(np.int32)
    shifts[0] = (0, 0)
    for bidi in (0, 2, -1):
        moved = moref.apply(biref.apply(frames, bidi, 0) if bidi else frames, shifts, 0)
        ext = WeightedTraceExtractor((H, W), T, frames.dtype, rois, weights, chunk_frames=16, shifts=shifts, bidi=bidi)
        for a in range(0, T, 16):
            ext.feed(frames[a:a + 16])
        assert np.array_equal(ext.result('sum'), ref.roi_sums(moved, rois, weights)), bidi
    ext = WeightedTraceExtractor((H, W), T, frames.dtype, rois, weights, bidi=3).feed(frames)
    assert np.array_equal(ext.result('sum'), ref.roi_sums(biref.apply(frames, 3, 0), rois, weights))


def test_all_256_weights_are_256_times_the_unweighted_extractor():
    from deep_calcium_amd import RoiTraceExtractor, WeightedTraceExtractor
    frames, rois, _ = _recording()
    T, H, W = frames.shape
    plain = RoiTraceExtractor((H, W), T, frames.dtype, rois).feed(frames)
    wtd = WeightedTraceExtractor((H, W), T, frames.dtype, rois, [np.full(len(c), 256) for c in rois]).feed(frames)
    assert np.array_equal(wtd.result('sum'), 256 * plain.result('sum'))
    assert wtd.areas_host().tolist() == (256 * plain.areas_host()).tolist()
    for kind in ('mean', 'zscore'):
        a, b = wtd.result(kind), plain.result(kind)
        assert a.dtype == np.float32 and a.tobytes() == b.tobytes(), kind


# ---- 4. downstream: unchanged kernels on the new input ---------------------------------------------------------------------------
def test_baseline_and_trace_pairs_take_the_weight_sums_as_areas():
    from deep_calcium_amd import TraceBaseline, TracePairCorr, WeightedTraceExtractor
    frames, rois, weights = _recording()
    T, H, W = frames.shape
    ext = WeightedTraceExtractor((H, W), T, frames.dtype, rois, weights).feed(frames)
    S = ref.roi_sums(frames, rois, weights)
    Wsum = np.array(ref.weight_sums(weights), np.int64)
    mean = ext.result('mean')
    assert mean.tobytes() == (S / Wsum[:, None].astype(np.float64)).astype(np.float32).tobytes()       # the weighted mean
    tb = TraceBaseline(ext.sums_device(), ext.areas_host(), 9, percentile=20, offset=40000)
    N, D = dref.numerators(S, Wsum, offset=40000)
    assert np.array_equal(tb.result('num'), N) and tb.denominators().tolist() == D.tolist()
    base = dref.baseline(N, 4, 20)
    assert np.array_equal(tb.result('baseline_sum'), base)
    assert tb.result('dff').tobytes() == dref.dff(N, base).tobytes()
    pairs = [(0, 1), (1, 2), (2, 0), (1, 1)]
    got = TracePairCorr(ext.sums_device(), ext.areas_host(), pairs).result('moments')
    want = mref.moments([row.tolist() for row in S], pairs, None)
    assert [(m['Nxx'], m['Nxy'], m['Nyy']) for m in got] == want


# ---- 5. the one-call functions ---------------------------------------------------------------------------------------------------
def _dataset(tmp_path):
    """40 frames of 20 x 24 and three ROIs: 0 and 1 overlap in a 3 x 2 patch, 2 stands alone."""
    rs = np.random.RandomState(44)
    T, H, W = 40, 20, 24
    raw = rs.randint(100, 3000, size=(T, H, W)).astype(np.int16)
    boxes = [(3, 8, 3, 9), (5, 10, 7, 13), (13, 17, 15, 20)]               # y0, y1, x0, x1
    rois = [np.array([[y, x] for y in range(y0, y1) for x in range(x0, x1)]) for y0, y1, x0, x1 in boxes]
    weights = [rs.randint(1, 257, len(c)) for c in rois]
    path = str(tmp_path / 'rec.npz')
    np.savez(path, series_raw=raw)
    return path, raw, rois, weights


def test_weighted_traces_device_keep_exclude_demix(tmp_path):
    from deep_calcium_amd import weighted_traces_device
    path, raw, rois, weights = _dataset(tmp_path)
    shape = raw.shape[1:]
    S = ref.roi_sums(raw, rois, weights)
    Wsum = np.array(ref.weight_sums(weights), np.float64)
    assert np.array_equal(weighted_traces_device(path, rois, weights, kind='sum', chunk_frames=7), S)
    assert weighted_traces_device(path, rois, weights).tobytes() == (S / Wsum[:, None]).astype(np.float32).tobytes()
    assert np.array_equal(weighted_traces_device(path, rois, kind='sum'), ref.roi_sums(raw, rois, None))        # weights=None: weight 1
    xr, xw, kept = ref.exclude_overlap(rois, weights)
    assert kept == [0, 1, 2] and len(xr[0]) == len(rois[0]) - 6
    assert np.array_equal(weighted_traces_device(path, rois, weights, kind='sum', overlap='exclude', chunk_frames=16), ref.roi_sums(raw, xr, xw))
    assert np.array_equal(weighted_traces_device(path, rois, kind='sum', overlap='exclude'), ref.roi_sums(raw, xr, None))
    # demix: numpy's float64 solve on integers that are IDENTICAL to the oracle's (the sums and the Gram matrix are exact), against
    # the oracle's exact rational solution rounded once.  Not equality: the LU factorisation rounds at every step, a relative
    # error of a few ulp times the condition number of a 2 x 2 Gram matrix of overlapping boxes (below 10); 1e-12 leaves four
    # decimal orders of room over that and would still catch a wrong weight or pixel, which moves a coefficient by parts in 10^3.
    G = ref.gram(rois, weights)
    want = ref.demix(S, G)
    got = weighted_traces_device(path, rois, weights, kind='demix', overlap='demix')
    assert got.dtype == np.float64 and got.shape == S.shape
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.array_equal(got[2], S[2] / np.float64(G[2][2]))                                   # the ROI that shares nothing
    z = weighted_traces_device(path, rois, weights, kind='zscore', overlap='demix')
    d = want - want.mean(1, keepdims=True)
    assert np.allclose(z, d / np.sqrt((d * d).mean(1, keepdims=True)), rtol=1e-10, atol=1e-10)
    gotb = weighted_traces_device(path, rois, kind='demix', overlap='demix')
    wantb = ref.demix(ref.roi_sums(raw, rois, None), ref.gram(rois))
    assert np.abs(gotb - wantb).max() <= 1e-12 * np.abs(wantb).max()


def test_dff_traces_device_with_weights(tmp_path):
    from deep_calcium_amd import dff_traces_device
    path, raw, rois, weights = _dataset(tmp_path)
    shape = raw.shape[1:]
    S = ref.roi_sums(raw, rois, weights)
    Wsum = np.array(ref.weight_sums(weights), np.int64)
    N, D = dref.numerators(S, Wsum)
    assert np.array_equal(dff_traces_device(path, rois, 7, kind='num', weights=weights), N)
    assert dff_traces_device(path, rois, 7, percentile=30, weights=weights, chunk_frames=9).tobytes() == dref.dff(N, dref.baseline(N, 3, 30)).tobytes()
    # rings stay unweighted: their sums are plain sums, their areas pixel counts
    rings = dref.rings(rois, shape, 1, 4)
    assert all(len(r) for r in rings)
    Sn = ref.roi_sums(raw, rings, None)
    An = np.array([len(r) for r in rings], np.int64)
    N, D = dref.numerators(S, Wsum, Sn, An, 0.7, 0)
    assert np.array_equal(dff_traces_device(path, rois, 7, kind='num', neuropil=(1, 4, 0.7), weights=weights), N)
    got = dff_traces_device(path, rois, 7, neuropil=(1, 4, 0.7), weights=weights)
    assert got.tobytes() == dref.dff(N, dref.baseline(N, 3, 8)).tobytes()
    # weights=None: the unweighted path, as before
    Nb, _ = dref.numerators(ref.roi_sums(raw, rois, None), np.array([len(c) for c in rois], np.int64))
    assert np.array_equal(dff_traces_device(path, rois, 7, kind='num'), Nb)


# ---- 6. the tape trampoline ------------------------------------------------------------------------------------------------------
def test_entry_point_replayed_from_a_tape_gives_the_same_bytes(dclib):
    from deep_calcium_amd._lib import Tape
    rs = np.random.RandomState(3)
    H, W, tc, t0 = 7, 9, 33, 2
    off, pix, wgt = _small_csr(rs, H * W)
    roi = [1, 0, 1, 2, 7]
    frames = _frames(rs, (tc, H, W), np.int16)
    f = torch.from_numpy(frames).cuda()
    w = torch.from_numpy(wgt.astype(np.uint16).view(np.int16)).cuda()
    d_off, d_pix, d_roi = _i32(off), _i32(pix), _i32(roi)
    sums = torch.full((4, t0 + tc), GARBAGE, dtype=torch.int64, device='cuda')
    args = (f.data_ptr(), 0, tc, t0, d_off.data_ptr(), d_pix.data_ptr(), w.data_ptr(), d_roi.data_ptr(), 5, 4, sums.data_ptr(), t0 + tc, H, W, _st())
    dclib.dc_roi_wtrace_accumulate(*args)
    torch.cuda.synchronize()
    direct = sums.cpu().numpy()
    assert direct[:, t0:].tolist() == ref.csr_sums(frames, off, pix, wgt, roi, 4)
    sums.fill_(GARBAGE)
    tape = Tape(dclib, [('dc_roi_wtrace_accumulate', args)])
    tape.replay({})
    torch.cuda.synchronize()
    assert sums.cpu().numpy().tobytes() == direct.tobytes()


# ---- 7. the command ----------------------------------------------------------------------------------------------------------------
def test_example_traces_command_with_weighted(tmp_path, monkeypatch):
    """examples/neurons/unet2ds_nf.py `traces --weighted`: the final ROIs -> one more footprint pass -> footprint_weights -> weighted
    traces.  The prediction is stood in for by the planted mask; the footprint correlations are the product's own (tested in
    test_footprints_gpu.py), everything behind them is compared with the oracle."""
    import importlib.util
    import os
    from deep_calcium_amd import UNet2DSummary, hdf5_min, roi_footprints_device
    rs = np.random.RandomState(12)
    T, H, W = 60, 24, 32
    raw = rs.randint(300, 500, size=(T, H, W)).astype(np.float64)
    mask2d = np.zeros((H, W), np.float32)
    yy, xx = np.mgrid[:H, :W]
    for cy, cx in ((6, 7), (15, 22)):
        prof = np.exp(-(((yy - cy) / 2.5) ** 2 + ((xx - cx) / 2.5) ** 2))
        raw += rs.randint(0, 800, size=T)[:, None, None] * prof[None]
        mask2d[prof > 0.1] = 0.9                              # wider than the cell: the rim barely follows the trace
    raw = np.rint(raw).astype(np.int16)
    path = str(tmp_path / 'rec.npz')
    np.savez(path, series_raw=raw, series_mean=raw.mean(0).astype(np.float16), name=np.array('neurofinder.00.00'))
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'neurons', 'unet2ds_nf.py')
    state = np.random.get_state()                             # the example seeds numpy's global stream on import
    try:
        spec = importlib.util.spec_from_file_location('example_unet2ds_nf_weighted', script)
        example = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(example)
    finally:
        np.random.set_state(state)
    monkeypatch.setattr(UNet2DSummary, 'predict', lambda self, dspaths, **kw: ([mask2d], ['neurofinder.00.00']))
    corr, coords, inside = roi_footprints_device(path, mask2d.round().astype(np.uint8), halo=0)
    floor = 0.5
    rois, weights, kept = ref.footprint_weights(coords, corr, inside, floor)
    assert kept == [0, 1] and 0 < sum(len(r) for r in rois) < sum(len(c) for c in coords) and len(set(weights[0])) > 3
    S = ref.roi_sums(raw, rois, weights)
    Wsum = np.array(ref.weight_sums(weights), np.int64)

    def run(**kw):
        cp = str(tmp_path / ('cp_' + '_'.join('%s' % v for v in kw.values())))
        example.traces([path], None, cp, weighted=floor, **kw)
        with hdf5_min.File(os.path.join(cp, 'neurofinder.00.00_traces.hdf5')) as f:
            return f['traces'].read()
    assert np.array_equal(run(kind='sum'), S)
    assert np.array_equal(run(kind='sum', overlap='exclude'), S)                              # regions of one mask share nothing
    assert run(kind='mean').tobytes() == (S / Wsum[:, None].astype(np.float64)).astype(np.float32).tobytes()
    G = ref.gram(rois, weights)
    assert np.array_equal(run(kind='mean', overlap='demix'), np.stack([S[r] / np.float64(G[r][r]) for r in range(2)]))
    N, _ = dref.numerators(S, Wsum)
    assert run(dff=9).tobytes() == dref.dff(N, dref.baseline(N, 4, 8)).tobytes()
    for kw, what in ((dict(weighted=0.0, overlap='demix', dff=9), 'not together'), (dict(overlap='exclude'), 'needs --weighted'),
                     (dict(weighted=float('nan')), 'FLOOR'), (dict(weighted=0.0, overlap='both'), '--overlap is')):
        with pytest.raises(ValueError, match=what):
            example.traces([path], None, str(tmp_path / 'cp_err'), **kw)
