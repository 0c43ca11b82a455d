"""ROI traces on the device (include/dcunet.h dc_roi_trace_accumulate / dc_roi_trace_finalize; deep_calcium_amd/traces.py) against
numpy integers and an exact-integer / 60-digit decimal reference computed here."""
import decimal

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

from test_series_gpu import _frames, _ulps      # noqa: E402  the full-range frames and the float32 distance of the series tests

SHAPES = [(1, 1), (5, 7), (33, 19), (16, 64)]
TS = [1, 3, 37]
GARBAGE = -0x0123456789abcdef


def _seg():
    from deep_calcium_amd.traces import SEGMENT_PIXELS
    return SEGMENT_PIXELS


def _roi_rows(H, W):
    """The pixel lists of one image, as the C ABI takes them (int32 flat indices): sorted random subsets of every length at which
    the kernel changes path, plus what only the ABI allows -- an index twice, an empty row, indices outside the image."""
    n = H * W
    rs = np.random.RandomState(7 * H + W)
    S = _seg()
    rows = [np.array([n - 1])]                                              # a single pixel (the last one)
    rows.append(np.array([0]))                                              # _frames holds pixel 0 constant in time
    for k in (63, 64, 65, S - 1, S, S + 1, 2 * S + 3):
        if k <= n:
            rows.append(np.sort(rs.choice(n, k, replace=False)))
    rows.append(np.arange(0, min(n, 10)))                                   # two that overlap
    rows.append(np.arange(min(n - 1, 5), min(n, 15)))
    same = np.sort(rs.choice(n, min(n, 20), replace=False))
    rows += [same, same.copy()]                                             # two identical
    rows.append(np.array([0, 0, n - 1]))                                    # an index listed twice counts twice
    rows.append(np.zeros(0, np.int64))                                      # an empty row
    rows.append(np.array([n, -1, 0, 2 ** 31 - 1, -2 ** 31, n // 2]))        # H*W, -1 and the int32 extremes contribute 0
    return [np.asarray(r, np.int32) for r in rows]


def _sums_ref(frames, rows):
    T = frames.shape[0]
    x = frames.astype(np.int64).reshape(T, -1)
    out = np.zeros((len(rows), T), np.int64)
    for r, pix in enumerate(rows):
        pix = pix[(pix >= 0) & (pix < x.shape[1])]
        out[r] = x[:, pix].sum(1)
    return out


def _areas(rows, n):
    return np.array([int(((p >= 0) & (p < n)).sum()) for p in rows], np.int32)


class _Csr(object):
    """ROIs as device CSR arrays: whole (row_roi null: CSR row s is ROI s) or cut into segments of `split` pixels."""

    def __init__(self, rows, split=None):
        self.R = len(rows)
        if split is None:
            parts, owner = rows, None
        else:
            parts, owner = [], []
            for r, pix in enumerate(rows):
                for a in range(0, len(pix), split):
                    parts.append(pix[a:a + split])
                    owner.append(r)
        self.S = len(parts)
        off = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int32)
        pix = np.concatenate(parts + [np.zeros(1, np.int32)]).astype(np.int32)      # never empty: a null pointer is an error
        self.off, self.pix = torch.from_numpy(off).cuda(), torch.from_numpy(pix).cuda()
        self.roi = torch.from_numpy(np.asarray(owner + [0], np.int32)).cuda() if split is not None else None


class _Traces(object):
    """The raw C ABI on caller-owned buffers: what a binding without deep_calcium_amd/traces.py would do."""

    def __init__(self, dclib, H, W, csr, T, pad=3):
        self.L, self.H, self.W, self.csr, self.T, self.ld = dclib, H, W, csr, T, T + pad
        # filled with garbage on purpose: every call must write its own columns of every row and nothing else
        self.sums = torch.full((csr.R, self.ld), GARBAGE, dtype=torch.int64, device='cuda')

    def feed(self, dframes, uns, t0, tc):
        c = self.csr
        self.L.dc_roi_trace_accumulate(dframes[t0:t0 + tc].data_ptr(), uns, tc, t0, c.off.data_ptr(), c.pix.data_ptr(),
                                       c.roi.data_ptr() if c.roi is not None else None, c.S, c.R, self.sums.data_ptr(), self.ld,
                                       self.H, self.W, torch.cuda.current_stream().cuda_stream)

    def run(self, dframes, uns, chunk):
        for t0 in range(0, self.T, chunk):
            self.feed(dframes, uns, t0, min(chunk, self.T - t0))
        torch.cuda.synchronize()
        return self.sums.cpu().numpy()

    def finalize(self, areas, mean=True, zscore=True):
        out = torch.full((2, self.csr.R, self.T), float('nan'), dtype=torch.float32, device='cuda')
        a = torch.from_numpy(np.asarray(areas, np.int32)).cuda()
        self.L.dc_roi_trace_finalize(self.sums.data_ptr(), self.ld, a.data_ptr(), self.csr.R, self.T,
                                     out[0].data_ptr() if mean else None, out[1].data_ptr() if zscore else None,
                                     torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return out[0].cpu().numpy(), out[1].cpu().numpy()


def _device_frames(frames):
    return torch.from_numpy(np.ascontiguousarray(frames).view(np.int16)).cuda()


# ---- 1. sums -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.int16, np.uint16], ids=['int16', 'uint16'])
@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%d' % s for s in SHAPES])
def test_sums_equal_numpy_for_every_chunking_and_every_split(dclib, shape, dtype):
    H, W = shape
    rows = _roi_rows(H, W)
    uns = int(dtype == np.uint16)
    data = []
    for T in TS:
        frames = _frames(T, H, W, dtype)
        assert H * W == 1 or set(frames.ravel().tolist()) >= {np.iinfo(dtype).min, np.iinfo(dtype).max}
        data.append((T, _device_frames(frames), _sums_ref(frames, rows)))
    for split in (None, 1, 7, _seg()):
        csr = _Csr(rows, split)
        for T, dframes, want in data:
            for chunk in sorted({1, 2, 16, T}):
                tag = (split, T, chunk)
                st = _Traces(dclib, H, W, csr, T)
                if chunk < T:                    # after the first chunk only: every later column keeps its garbage
                    st.feed(dframes, uns, 0, chunk)
                    torch.cuda.synchronize()
                    part = st.sums.cpu().numpy()
                    assert np.array_equal(part[:, :chunk], want[:, :chunk]) and (part[:, chunk:] == GARBAGE).all(), tag
                got = st.run(dframes, uns, chunk)
                assert np.array_equal(got[:, :T], want), tag
                assert (got[:, T:] == GARBAGE).all(), tag          # ld > T: the padding is not touched


def test_no_32_bit_accumulator_anywhere(dclib):
    """260 x 256 = 66560 pixels at the types' extremes: 66560 * 65535 = 4 362 009 600 and 66560 * -32768 = -2 181 038 080 per
    frame, both beyond int32 -- as one row walked by one workgroup, and cut into segments beside 300 small ROIs and one of
    2 * SEGMENT_PIXELS + 3 pixels."""
    from deep_calcium_amd.traces import rois_to_csr
    H, W, T = 260, 256, 2
    n = H * W
    whole = np.arange(n, dtype=np.int32)
    for dtype, value, total in ((np.uint16, 65535, 4362009600), (np.int16, -32768, -2181038080)):
        frames = np.full((T, H, W), value, dtype)
        got = _Traces(dclib, H, W, _Csr([whole]), T).run(_device_frames(frames), int(dtype == np.uint16), T)
        assert got[:, :T].tolist() == [[total, total]] and total == n * value and abs(total) > 2 ** 31
    rs = np.random.RandomState(3)
    rois = [whole] + [np.sort(rs.choice(n, rs.randint(100, 401), replace=False)).astype(np.int32) for _ in range(300)]
    rois.append(np.sort(rs.choice(n, 2 * _seg() + 3, replace=False)).astype(np.int32))
    frames = rs.randint(0, 65536, size=(T, H, W)).astype(np.uint16)
    frames[0] = 65535
    want = _sums_ref(frames, rois)
    assert want[0, 0] == 4362009600
    areas, off, pix, roi = rois_to_csr([np.stack(np.unravel_index(p, (H, W)), 1) for p in rois], (H, W))
    assert areas.tolist() == [len(p) for p in rois] and len(roi) > len(rois) + n // _seg() - 1
    csr = _Csr(rois)                              # the buffers of the whole form, then replaced by the library's own split
    csr.S, csr.off, csr.pix, csr.roi = len(roi), torch.from_numpy(off).cuda(), torch.from_numpy(pix).cuda(), torch.from_numpy(roi).cuda()
    dframes = _device_frames(frames)
    got = _Traces(dclib, H, W, csr, T).run(dframes, 1, T)
    assert np.array_equal(got[:, :T], want)
    assert np.array_equal(_Traces(dclib, H, W, _Csr(rois), T).run(dframes, 1, 1)[:, :T], want)


# ---- 2. mean and z-score -------------------------------------------------------------------------------------------------
def _zscore_ref(sums):
    """(trace - mean) / population std along time from exact Python integers: (T S_t - sum S) / sqrt(T sum S^2 - (sum S)^2) in
    60-digit decimal arithmetic, one rounding at the end (decimal -> double -> float32; the double step moves the result by
    < 2^-29 float32 ulp).  A trace with zero variance: 0."""
    ctx = decimal.Context(prec=60)
    R, T = sums.shape
    out = np.zeros((R, T), np.float64)
    for r in range(R):
        s = [int(v) for v in sums[r]]
        s1, s2 = sum(s), sum(v * v for v in s)
        den = T * s2 - s1 * s1
        assert den >= 0
        if den == 0:
            continue
        root = ctx.sqrt(decimal.Decimal(den))
        out[r] = [float(ctx.divide(decimal.Decimal(T * v - s1), root)) for v in s]
    return out.astype(np.float32)


def _check_float_traces(st, sums, areas, T, tag):
    """mean bit-equal to numpy's; zscore within 1 float32 ulp of exact arithmetic and inside its mathematical range."""
    mean, z = st.finalize(areas)
    with np.errstate(divide='ignore', invalid='ignore'):
        want = np.where(areas[:, None] > 0, sums / areas[:, None], 0.0).astype(np.float32)
    assert np.array_equal(mean.view(np.int32), want.view(np.int32)), tag
    zref = _zscore_ref(np.where(areas[:, None] > 0, sums, 0))
    assert np.isfinite(z).all(), tag
    d = _ulps(z, zref)
    print('zscore %s: max %d ulp' % (tag, d.max()))
    assert d.max() <= 1, (tag, int(d.max()))
    # |z| <= sqrt(T - 1) for any T numbers (reached when one frame differs from all the others)
    assert np.abs(z).astype(np.float64).max() <= np.sqrt(T - 1.0), (tag, float(np.abs(z).max()))
    flat = (sums == sums[:, :1]).all(1) | (areas == 0)
    assert not z[flat].any() and not mean[areas == 0].any(), tag          # constant in time (T == 1 included): exactly 0
    # each output alone: the other buffer is not touched
    only_mean, nan = st.finalize(areas, zscore=False)
    assert np.array_equal(only_mean.view(np.int32), mean.view(np.int32)) and np.isnan(nan).all()
    nan, only_z = st.finalize(areas, mean=False)
    assert np.array_equal(only_z.view(np.int32), z.view(np.int32)) and np.isnan(nan).all()
    return z


@pytest.mark.parametrize('dtype', [np.int16, np.uint16], ids=['int16', 'uint16'])
@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%d' % s for s in SHAPES])
def test_mean_is_numpys_and_zscore_within_one_ulp_of_exact_arithmetic(dclib, shape, dtype):
    H, W = shape
    rows = _roi_rows(H, W)
    areas = _areas(rows, H * W)
    assert (areas == 0).any() and (areas == 1).any()
    for T in TS:
        frames = _frames(T, H, W, dtype, seed=1)
        st = _Traces(dclib, H, W, _Csr(rows, 7), T)
        sums = st.run(_device_frames(frames), int(dtype == np.uint16), 16)[:, :T]
        assert np.array_equal(sums, _sums_ref(frames, rows))
        z = _check_float_traces(st, sums, areas, T, (H, W, T, np.dtype(dtype).name))
        if T == 1:
            assert not z.any()
        if H * W > 1 and T > 1:
            assert not z[1].any()                # pixel 0 of _frames holds one value for all frames
            assert z.any()


def test_zscore_needs_the_128_bit_sums(dclib):
    """A whole-image ROI of a 260 x 256 uint16 recording that alternates between 0 and 65535: S^2 = 1.9e19 > 2^64 in every
    second frame, T sum S^2 = 1.3e22.  Beside it: half the image, and one pixel that is constant."""
    H, W, T = 260, 256, 37
    n = H * W
    frames = np.zeros((T, H, W), np.uint16)
    frames[1::2] = 65535
    frames[:, 0, 0] = 7
    frames[::3, H // 2:] //= 3
    rows = [np.arange(n, dtype=np.int32), np.arange(n // 2, n, dtype=np.int32), np.array([0], np.int32), np.arange(1, n, dtype=np.int32)]
    areas = _areas(rows, n)
    st = _Traces(dclib, H, W, _Csr(rows, _seg()), T)
    sums = st.run(_device_frames(frames), 1, 16)[:, :T]
    assert np.array_equal(sums, _sums_ref(frames, rows))
    assert int(sums[3, 1]) ** 2 > 2 ** 64
    z = _check_float_traces(st, sums, areas, T, 'alternating')
    assert not z[2].any()
    assert (z[3, 1::2] > 0).all() and (z[3, 0::2] < 0).all()


def test_constant_traces_and_single_frames_are_exactly_zero(dclib):
    H, W = 5, 7
    rows = [np.array([3], np.int32), np.arange(35, dtype=np.int32), np.array([0, 34, 34], np.int32)]
    areas = _areas(rows, 35)
    still = (np.arange(35).reshape(1, H, W) * 1800 - 32768).astype(np.int16)
    for T in (1, 2, 5):
        for frames in (np.repeat(still, T, 0), np.full((T, H, W), -32768, np.int16)):
            st = _Traces(dclib, H, W, _Csr(rows), T)
            sums = st.run(_device_frames(frames), 0, T)[:, :T]
            mean, z = st.finalize(areas)
            assert np.array_equal(z, np.zeros((3, T), np.float32)) and not np.signbit(z).any()
            assert np.array_equal(mean, (sums / areas[:, None]).astype(np.float32))
    # a moving sum over a constant one: T = 2 gives exactly -1 and +1
    frames = np.repeat(still, 2, 0)
    frames[1, 0, 3] += 1
    st = _Traces(dclib, H, W, _Csr(rows), 2)
    st.run(_device_frames(frames), 0, 1)
    assert st.finalize(areas)[1].tolist() == [[-1.0, 1.0], [-1.0, 1.0], [0.0, 0.0]]


# ---- 3. the product path -------------------------------------------------------------------------------------------------
def _dataset(tmp_path):
    """A small .npz dataset with planted neurons, as test_series_gpu._dataset makes it -- on a grid, so that no two overlap, and
    with the planted signals handed back."""
    rs = np.random.RandomState(4)
    T, H, W = 40, 48, 40
    raw = rs.randint(50, 400, size=(T, H, W))
    masks = np.zeros((6, H, W), np.int8)
    signals = rs.randint(0, 3000, size=(6, T))
    for z in range(6):
        cy, cx = 8 + 16 * (z // 2), 10 + 20 * (z % 2)
        masks[z, cy - 2:cy + 3, cx - 2:cx + 3] = 1
        raw[:, cy - 2:cy + 3, cx - 2:cx + 3] += signals[z][:, None, None]          # a neuron: pixels that move together
    raw = raw.astype(np.int16)
    p = str(tmp_path / 'rec.npz')
    np.savez(p, series_raw=raw, series_mean=raw.mean(0).astype(np.float16), masks_raw=masks, name=np.array('neurofinder.00.00'))
    return p, raw, masks, signals


def test_extract_traces_device_through_the_product_path(tmp_path):
    from deep_calcium_amd import RoiTraceExtractor, SeriesSummarizer, extract_traces_device
    from deep_calcium_amd.nf_metrics import mask_to_regions
    path, raw, masks, signals = _dataset(tmp_path)
    T, H, W = raw.shape
    x = raw.astype(np.int64).reshape(T, -1)
    want = np.stack([x[:, np.flatnonzero(m)].sum(1) for m in masks])
    for chunk_frames in (7, 16):
        got = extract_traces_device(path, masks, kind='sum', chunk_frames=chunk_frames)
        assert got.dtype == np.int64 and np.array_equal(got, want), chunk_frames
    # a recording that is already resident: one int16 CUDA tensor, read in place
    ext = RoiTraceExtractor((H, W), T, raw.dtype, masks)
    assert ext.areas.tolist() == [25] * 6
    ext.feed(torch.from_numpy(raw).cuda())
    assert ext._stage is None and np.array_equal(ext.result('sum'), want)
    # a summarizer alive and fed in between: its staging slots are its own
    ext = RoiTraceExtractor((H, W), T, raw.dtype, masks, chunk_frames=8)
    summ = SeriesSummarizer((H, W), T, raw.dtype, chunk_frames=8, kinds=('mean',))
    for a in range(0, T, 10):
        ext.feed(raw[a:a + 10])
        summ.feed(raw[a:a + 10])
    for k in range(2):
        assert ext._stage._host[k] is not summ._stage._host[k]
        assert ext._stage._host[k][0].data_ptr() != summ._stage._host[k][0].data_ptr()
    assert np.array_equal(ext.result('sum'), want)
    assert np.array_equal(summ.result('mean'), (x.sum(0) / float(T)).astype(np.float32).reshape(H, W))
    mean = ext.result('mean')
    assert mean.dtype == np.float32 and np.array_equal(mean, (want / 25.0).astype(np.float32))
    # a planted neuron's normalised trace follows its planted signal
    z = extract_traces_device(path, masks, kind='zscore')
    assert z.dtype == np.float32 and z.shape == (6, T)
    for r in range(6):
        assert np.corrcoef(z[r], signals[r])[0, 1] > 0.9, r
    assert np.abs(z.mean(1)).max() < 1e-5 and np.abs(z.std(1) - 1).max() < 1e-5
    # the 2-D mask predict() returns: one trace per mask_to_regions region, in its order
    mask2d = masks.max(0).astype(np.uint8)
    mask2d[0, 0] = mask2d[1, 1] = 1               # a region that holds together only diagonally, first in raster order
    regions = mask_to_regions(mask2d)
    assert len(regions) == 7 and len(regions[0]) == 2
    got = extract_traces_device(path, mask2d, kind='sum')
    assert np.array_equal(got, np.stack([raw[:, r[:, 0], r[:, 1]].astype(np.int64).sum(1) for r in regions]))
    uns = str(tmp_path / 'uns.npz')
    np.savez(uns, series_raw=(raw.astype(np.int32) + 40000).astype(np.uint16))
    assert np.array_equal(extract_traces_device(uns, masks, kind='sum', chunk_frames=16), want + 25 * 40000)


def test_example_traces_command_writes_the_spikes_models_file(tmp_path, monkeypatch):
    """examples/neurons/unet2ds_nf.py `traces`: mask -> regions -> traces of series/raw -> the traces file.  The prediction is
    stood in for by the planted masks (an untrained model predicts next to nothing); everything behind it is the command's own."""
    import importlib.util
    import os
    from deep_calcium_amd import UNet2DSummary, hdf5_min
    from deep_calcium_amd.nf_metrics import mask_to_regions
    path, raw, masks, _ = _dataset(tmp_path)
    mask2d = masks.max(0).astype(np.float32) * 0.9            # probabilities: the command rounds them
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'neurons', 'unet2ds_nf.py')
    state = np.random.get_state()                             # the example seeds numpy's global stream on import
    try:
        spec = importlib.util.spec_from_file_location('example_unet2ds_nf', script)
        example = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(example)
    finally:
        np.random.set_state(state)
    monkeypatch.setattr(UNet2DSummary, 'predict', lambda self, dspaths, **kw: ([mask2d, np.zeros_like(mask2d)], ['neurofinder.00.00', 'empty']))
    cp = str(tmp_path / 'cp')
    example.traces([path, path], None, cp, kind='sum')
    assert sorted(f for f in os.listdir(cp) if f.endswith('_traces.hdf5')) == ['neurofinder.00.00_traces.hdf5']
    regions = mask_to_regions(mask2d.round())
    with hdf5_min.File(os.path.join(cp, 'neurofinder.00.00_traces.hdf5')) as f:
        name = f.attrs['name']
        assert (name.decode() if isinstance(name, bytes) else str(name)) == 'neurofinder.00.00'
        got = f['traces'].read()
    assert got.dtype == np.int64 and len(regions) == 6
    assert np.array_equal(got, np.stack([raw[:, r[:, 0], r[:, 1]].astype(np.int64).sum(1) for r in regions]))


# ---- 4. errors -----------------------------------------------------------------------------------------------------------
def test_errors_are_raised_before_any_launch(dclib):
    from deep_calcium_amd import RoiTraceExtractor
    from deep_calcium_amd._lib import DcunetError
    rois = [np.array([[1, 2], [3, 4]]), np.array([[0, 0]])]
    e = RoiTraceExtractor((5, 7), 4, np.int16, rois)
    ok = np.zeros((2, 5, 7), np.int16)
    with pytest.raises(ValueError, match='uint16'):
        e.feed(ok.astype(np.uint16))
    with pytest.raises(ValueError, match=r'\(t, 5, 7\)'):
        e.feed(np.zeros((2, 7, 5), np.int16))
    with pytest.raises(ValueError, match='numpy array'):
        e.feed([ok])
    with pytest.raises(ValueError, match='torch.int16'):
        e.feed(torch.zeros((2, 5, 7), dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError, match='the tensor is on cpu'):
        e.feed(torch.zeros((2, 5, 7), dtype=torch.int16))
    with pytest.raises(ValueError, match='contiguous'):
        e.feed(torch.zeros((2, 5, 14), dtype=torch.int16, device='cuda')[:, :, ::2])
    with pytest.raises(ValueError, match='after 0 of 4'):
        e.result('mean')
    e.feed(ok)
    with pytest.raises(ValueError, match='declared to have 4'):
        e.feed(np.zeros((3, 5, 7), np.int16))
    assert e.fed == 2
    e.feed(torch.from_numpy(ok).cuda())
    with pytest.raises(ValueError, match='not one of'):
        e.result('median')
    assert e.result('sum').tolist() == [[0] * 4] * 2 and e.result('zscore').tolist() == [[0.0] * 4] * 2
    # the volume limit of the 128-bit z-score, on the C ABI itself: refused with DC_EUNSUP, nothing launched
    st = _Traces(dclib, 5, 7, _Csr([np.array([1, 2], np.int32)]), 4)
    before = st.sums.cpu().numpy()
    d = _device_frames(ok)
    c, stream = st.csr, torch.cuda.current_stream().cuda_stream
    T = 2 ** 46 // 35
    with pytest.raises(DcunetError, match=r'\(-3\).*70368744177664'):
        dclib.dc_roi_trace_accumulate(d.data_ptr(), 0, 1, T, c.off.data_ptr(), c.pix.data_ptr(), None, 1, 1, st.sums.data_ptr(), T + 1,
                                      5, 7, stream)
    with pytest.raises(DcunetError, match=r'\(-3\).*70368744177664'):
        dclib.dc_roi_trace_finalize(st.sums.data_ptr(), 2 ** 46 + 1, c.off.data_ptr(), 1, 2 ** 46 + 1, st.sums.data_ptr(), None, stream)
    with pytest.raises(DcunetError, match=r'\(-1\)'):
        dclib.dc_roi_trace_accumulate(d.data_ptr(), 0, 2, 3, c.off.data_ptr(), c.pix.data_ptr(), None, 1, 1, st.sums.data_ptr(), 4, 5, 7, stream)
    with pytest.raises(DcunetError, match=r'\(-1\)'):
        dclib.dc_roi_trace_accumulate(d.data_ptr(), 0, 2, 0, c.off.data_ptr(), c.pix.data_ptr(), None, 2, 1, st.sums.data_ptr(), 7, 5, 7, stream)
    torch.cuda.synchronize()
    assert np.array_equal(st.sums.cpu().numpy(), before) and (before == GARBAGE).all()
