"""ROI pixel-pair correlation on the device (include/dcunet.h dc_roi_pair_accumulate / dc_roi_pair_corr;
deep_calcium_amd/roi_pairs.py) against the Python-integer / 60-digit decimal reference of tests/_pair_ref.py, and the split of
merged ROIs on the scenes whose conditions tests/test_roi_pairs_api.py checks on the float64 oracle."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _pair_ref as ref                           # noqa: E402
from test_series_gpu import _frames, _ulps        # noqa: E402  the full-range frames and the float32 distance of the series tests

H, W, T = 12, 24, 50
BATCH = 32                                        # DC_ROI_PAIR_BATCH; test_constants_are_the_headers checks it
SENTINEL = 0x5a5a5a5a5a5a5a5a                      # what the lower triangles hold before and after
TWO62 = 1 << 62


def _layout():
    """The ROIs of the raw-ABI tests as flat pixel lists of a 12 x 24 frame: 1, 63, 64, 65 and 130 pixels (diagonal tiles,
    off-diagonal tiles, ragged last tiles), two that overlap, one twice, and one that holds pixel 0 (constant in time in _frames)
    and indices outside the image (which count as 0)."""
    n = H * W
    rs = np.random.RandomState(4)
    rois = [np.array([n - 1])] + [np.sort(rs.choice(n, k, replace=False)) for k in (63, 64, 65, 130)]
    rois += [np.arange(40, 110), np.arange(90, 160)]                              # overlapping
    rois += [rois[3].copy()]                                                      # the 65-pixel ROI again
    rois += [np.array([0, 1, 5, 7, n, -1, 2 ** 31 - 1, -2 ** 31, n // 2])]
    return [np.asarray(r, np.int32) for r in rois]


class _Dev(object):
    """The raw C ABI on caller-owned buffers: what a binding without deep_calcium_amd/roi_pairs.py would do.  The tile list
    carries tiles that name nothing (no ROI, tj < ti, beyond the ROI's last tile): they must change nothing."""

    def __init__(self, dclib, rois, h=H, w=W, junk=True):
        self.L, self.H, self.W, self.R = dclib, h, w, len(rois)
        self.k = [len(r) for r in rois]
        self.off, self.goff, tiles, self.G = ref.layout(self.k)
        self.P = self.off[-1]
        if junk:
            tiles = tiles + [(-1, 0, 0), (self.R, 0, 0), (4, 1, 0), (4, 3, 3), (4, 0, 3), (2 ** 31 - 1, 0, 0), (1, -1, 0)]
        self.ntiles = len(tiles)
        cuda = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).cuda()      # noqa: E731
        self.d_off, self.d_pix = cuda(self.off, np.int32), cuda(np.concatenate(rois), np.int32)
        self.d_goff, self.d_tiles = cuda(self.goff, np.int64), cuda(np.array(tiles, np.int64).reshape(-1, 3), np.int32)
        self.a0 = np.zeros(self.P, np.int64)
        self.g0 = np.zeros(self.G + 2, np.int64)                                  # two words beyond the state: never touched
        self.g0[self.G:] = SENTINEL
        self.lower = np.zeros(self.G + 2, bool)
        for go, k in zip(self.goff, self.k):
            self.lower[go:go + k * k] = np.tril(np.ones((k, k), bool), -1).ravel()
        self.g0[self.lower] = SENTINEL
        self.reset()

    def reset(self):
        self.a = torch.from_numpy(self.a0).cuda()
        self.g = torch.from_numpy(self.g0).cuda()

    def _st(self):
        return torch.cuda.current_stream().cuda_stream

    def feed(self, dframes, uns, t0, tc):
        self.L.dc_roi_pair_accumulate(dframes[t0:t0 + tc].data_ptr(), uns, tc, self.d_off.data_ptr(), self.d_pix.data_ptr(),
                                      self.d_goff.data_ptr(), self.d_tiles.data_ptr(), self.ntiles, self.R, self.a.data_ptr(),
                                      self.g.data_ptr(), self.P, self.G, self.H, self.W, self._st())

    def run(self, dframes, uns, chunks):
        self.reset()
        t0 = 0
        for tc in chunks:
            self.feed(dframes, uns, t0, tc)
            t0 += tc
        torch.cuda.synchronize()
        return self.moments()

    def moments(self):
        """-> (a, g) as numpy int64; asserts that the lower triangles and the words beyond the state still hold the sentinel."""
        a, g = self.a.cpu().numpy(), self.g.cpu().numpy()
        assert (g[self.lower] == SENTINEL).all() and (g[self.G:] == SENTINEL).all()
        return a, g

    def upper(self, g):
        """Per ROI the (k, k) square of g with the lower triangle zeroed."""
        return [np.triu(g[go:go + k * k].reshape(k, k)) for go, k in zip(self.goff, self.k)]

    def corr(self, n_frames):
        out = torch.full((self.G + 2,), float('nan'), dtype=torch.float32, device='cuda')
        self.L.dc_roi_pair_corr(self.a.data_ptr(), self.g.data_ptr(), self.d_off.data_ptr(), self.d_goff.data_ptr(), self.R, self.P, self.G,
                                n_frames, out.data_ptr(), self._st())
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert np.isnan(out[self.G:]).all() and np.isfinite(out[:self.G]).all()      # every entry of every square, nothing beyond
        return [out[go:go + k * k].reshape(k, k) for go, k in zip(self.goff, self.k)]


def _device_frames(frames):
    return torch.from_numpy(np.ascontiguousarray(frames).view(np.int16)).cuda()


def _inside(flat, n):
    return [int(p) if 0 <= p < n else None for p in flat]


def _moments_ref(frames, rois):
    """Per ROI (a, g) in Python integers; an index outside the image is a pixel that is always 0."""
    n = frames.shape[1] * frames.shape[2]
    out = []
    for r in rois:
        keep = [p for p in _inside(r, n) if p is not None]
        a, g = ref.moments(frames, keep)
        pos = [None if p is None else keep.index(p) for p in _inside(r, n)]
        k = len(r)
        out.append(([0 if pos[i] is None else a[pos[i]] for i in range(k)],
                    [[0 if pos[i] is None or pos[j] is None else g[pos[i]][pos[j]] for j in range(k)] for i in range(k)]))
    return out


@functools.lru_cache(maxsize=None)
def _case(dtype_name):
    """Frames, ROIs and the Python-integer reference, computed once and shared."""
    frames = _frames(T, H, W, np.dtype(dtype_name).type)
    rois = _layout()
    return frames, rois, _moments_ref(frames, rois)


def _check_moments(st, got, want, what):
    a, g = got
    for r, ((wa, wg), sq) in enumerate(zip(want, st.upper(g))):
        assert a[st.off[r]:st.off[r + 1]].tolist() == wa, (what, r, 'a')
        assert np.array_equal(sq.astype(object), np.triu(np.array(wg, object).reshape(len(wa), len(wa)))), (what, r, 'g')


def test_constants_are_the_headers():
    from deep_calcium_amd import roi_pairs
    assert roi_pairs.BATCH == BATCH and roi_pairs.TILE == ref.TILE == 64


# ---- 1. the raw ABI: moments exact ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.int16, np.uint16], ids=['int16', 'uint16'])
def test_moments_equal_python_integers_for_every_chunking(dclib, dtype):
    frames, rois, want = _case(np.dtype(dtype).name)
    assert [len(r) for r in rois][:5] == [1, 63, 64, 65, 130]
    dframes = _device_frames(frames)
    st = _Dev(dclib, rois)
    first = None
    for chunks in ([T], [1] * T, [BATCH - 1, T - BATCH + 1], [BATCH, T - BATCH], [BATCH + 1, T - BATCH - 1], [T]):
        got = st.run(dframes, int(dtype == np.uint16), chunks)
        _check_moments(st, got, want, chunks)
        first = got if first is None else first
        assert np.array_equal(first[0], got[0]) and np.array_equal(first[1], got[1])
    # the duplicate ROI holds what the ROI it repeats holds; a product of two pixels reaches beyond 32 bits
    sq = st.upper(got[1])
    assert np.array_equal(sq[3], sq[7]) and max(max(abs(v) for v in row) for row in want[4][1]) > 2 ** 32


@pytest.mark.parametrize('value,dtype', [(65535, np.uint16), (-32768, np.int16)], ids=['65535', '-32768'])
def test_extreme_pixels_for_a_full_chunk(dclib, value, dtype):
    """Every pixel at the value whose square is the largest product: 65535^2 > 2^31 (no product, and no run of products, fits 32
    bits), for two full batches of frames, in ROIs on both sides of the tile edge."""
    n_frames = 2 * BATCH
    frames = np.full((n_frames, H, W), value, dtype)
    rois = [np.arange(0, 65, dtype=np.int32), np.arange(100, 230, dtype=np.int32), np.array([287], np.int32)]
    st = _Dev(dclib, rois)
    a, g = st.run(_device_frames(frames), int(dtype == np.uint16), [n_frames])
    assert (a == value * n_frames).all()
    for sq, k in zip(st.upper(g), st.k):
        assert np.array_equal(sq, np.triu(np.full((k, k), value * value * n_frames, np.int64)))
    corr = st.corr(n_frames)
    assert all(not c.any() for c in corr)                                         # every pixel constant in time: exactly 0


@pytest.mark.parametrize('dtype', [np.int16, np.uint16], ids=['int16', 'uint16'])
def test_state_near_two_to_the_62_is_added_to_exactly(dclib, dtype):
    """State written by the test through the C ABI: +-2^62 and values near it, then one chunk of full-range frames on top.  The
    sums stay inside int64 (|chunk's g| < 2^32 * 50) and must come out exact: the kernel reads, adds and writes 64 bits."""
    frames, rois, want = _case(np.dtype(dtype).name)
    st = _Dev(dclib, rois)
    rs = np.random.RandomState(12)
    pre_a = rs.choice([TWO62, -TWO62, TWO62 - 1, 1 - TWO62, 2 ** 32, -1], size=st.P).astype(np.int64)
    pre_g = rs.choice([TWO62, -TWO62, TWO62 - 1, 1 - TWO62, 2 ** 32, -1], size=st.G + 2).astype(np.int64)
    st.a0 = pre_a
    st.g0 = np.where(st.lower | (np.arange(st.G + 2) >= st.G), st.g0, pre_g)
    a, g = st.run(_device_frames(frames), int(dtype == np.uint16), [T])
    for r, ((wa, wg), sq, pre) in enumerate(zip(want, st.upper(g), st.upper(pre_g))):
        k = len(wa)
        assert [int(v) for v in a[st.off[r]:st.off[r + 1]]] == [int(p) + v for p, v in zip(pre_a[st.off[r]:st.off[r + 1]], wa)], r
        assert np.array_equal(sq.astype(object), np.triu(pre.astype(object) + np.array(wg, object).reshape(k, k))), r
    assert max(abs(int(v)) for v in g[:st.G][~st.lower[:st.G]]) > TWO62


# ---- 2. corr ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.int16, np.uint16], ids=['int16', 'uint16'])
def test_corr_is_within_one_ulp_of_exact_arithmetic(dclib, dtype):
    frames, rois, want = _case(np.dtype(dtype).name)
    st = _Dev(dclib, rois)
    st.run(_device_frames(frames), int(dtype == np.uint16), [T])
    got = st.corr(T)
    worst = 0
    for r, (c, (a, g)) in enumerate(zip(got, want)):
        k = len(a)
        assert np.array_equal(c.view(np.int32), c.T.view(np.int32)), r              # bit-symmetric
        assert np.abs(c).max() <= 1.0
        varies = np.array([(a[i] * a[i] != T * g[i][i]) for i in range(k)])
        assert np.array_equal(np.diag(c), varies.astype(np.float32)), r              # the diagonal: exactly 1, or 0 for a constant pixel
        assert not c[~varies].any() and not c[:, ~varies].any() and not np.signbit(c[~varies]).any()
        exact = np.array([[ref.corr_exact(T, a, g, i, j) if i <= j else 0 for j in range(k)] for i in range(k)], np.float32).reshape(k, k)
        worst = max(worst, int(_ulps(np.triu(c), exact).max()))
    print('corr %s: max %d ulp of exact' % (np.dtype(dtype).name, worst))
    assert worst <= 1
    assert not got[8][0].any() and not got[8][4].any() and got[8][2, 2] == 1       # pixel 0 is constant; an index outside the image too
    # T == 1: every pixel is constant
    st.run(_device_frames(frames), int(dtype == np.uint16), [1])
    assert all(not c.any() for c in st.corr(1))


def test_corr_of_equal_and_negated_series_is_plus_and_minus_one(dclib):
    frames = _frames(37, 5, 7, np.int16, seed=2) // 4
    x = frames.reshape(37, -1)
    p, q, m, k = 17, 30, 9, 20
    x[:, q] = x[:, p]                                                               # equal
    x[:, m] = -x[:, p]                                                              # negated
    x[:, k] = -77                                                                   # constant
    st = _Dev(dclib, [np.array([m, 12, p, k, q], np.int32)], h=5, w=7, junk=False)
    st.run(_device_frames(frames), 0, [20, 17])
    c = st.corr(37)[0]
    assert c[2].tolist()[0] == -1.0 and c[2].tolist()[2:] == [1.0, 0.0, 1.0] and 0 < abs(c[2, 1]) < 1
    assert c[0, 4] == -1.0 and c[4, 0] == -1.0 and not c[3].any() and not c[:, 3].any()
    assert np.diag(c).tolist() == [1.0, 1.0, 1.0, 0.0, 1.0]


# ---- 3. the Python API -------------------------------------------------------------------------------------------------------
def _same_lists(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)


def _recording():
    rs = np.random.RandomState(6)
    n_frames, h, w = 12, 24, 24
    raw = rs.randint(-300, 3000, size=(n_frames, h, w)).astype(np.int16)
    rois = [np.argwhere(np.pad(np.ones((4, 5), bool), ((3, 17), (2, 17)))), np.array([[0, 0], [0, 1], [1, 0]]),
            np.argwhere(np.pad(np.ones((9, 9), bool), ((5, 10), (5, 10)))), np.array([[23, 23]])]      # 20, 3, 81 (two tiles) and 1 pixels
    for r in rois[:3]:
        raw[:, r[:, 0], r[:, 1]] += rs.randint(0, 2000, size=(n_frames, 1)).astype(np.int16)
    return raw, rois


def _check_against_reference(pc, frames, rois):
    n_frames, h, w = frames.shape
    _same_lists(pc.pixels(), [np.asarray(r, np.int64) for r in rois])
    got_m, got_c = pc.result('moments'), pc.result('corr')
    for r, roi in enumerate(rois):
        a, g = ref.moments(frames, [int(y) * w + int(x) for y, x in roi])
        assert got_m[r]['a'].dtype == object and got_m[r]['g'].dtype == object
        assert got_m[r]['a'].tolist() == a and got_m[r]['g'].tolist() == g, r       # g comes back whole and symmetric
        assert got_c[r].dtype == np.float32 and got_c[r].shape == (len(roi), len(roi))
        assert _ulps(got_c[r], ref.matrix(n_frames, a, g)).max() <= 1, r
        assert np.array_equal(got_c[r].view(np.int32), got_c[r].T.view(np.int32))
    return got_c


def test_class_numpy_chunks_resident_tensor_and_file_agree(tmp_path):
    from deep_calcium_amd import RoiPairCorr, RoiTraceExtractor, roi_pair_corr_device
    raw, rois = _recording()
    n_frames, h, w = raw.shape
    pc = RoiPairCorr((h, w), n_frames, raw.dtype, rois, chunk_frames=5)
    assert pc.n_tiles == 1 + 1 + 3 + 1 and pc.n_state == 400 + 9 + 81 * 81 + 1
    assert pc.feed(raw[:7]) is pc
    pc.feed(raw[7:])
    corr = _check_against_reference(pc, raw, rois)
    assert corr[3].tolist() == [[1.0]]
    ext = RoiTraceExtractor((h, w), n_frames, raw.dtype, rois).feed(raw)
    assert np.array_equal(pc.traces('sum'), ext.result('sum'))
    assert np.array_equal(pc.traces('zscore').view(np.int32), ext.result('zscore').view(np.int32))
    assert np.array_equal(pc.traces().view(np.int32), ext.result('mean').view(np.int32))
    assert ext._stage._host[0] is not pc._ext._stage._host[0]                   # staging slots of its own
    res = RoiPairCorr((h, w), n_frames, raw.dtype, rois)
    with pytest.raises(ValueError, match='after 0 of 12'):
        res.result('corr')
    res.feed(torch.from_numpy(raw).cuda())
    with pytest.raises(ValueError, match='not one of'):
        res.result('coherence')
    _same_lists(res.result('corr'), corr)
    assert res.result('moments')[2]['g'].tolist() == pc.result('moments')[2]['g'].tolist()
    path = str(tmp_path / 'rec.npz')
    np.savez(path, series_raw=raw)
    got = roi_pair_corr_device(path, rois, chunk_frames=4)
    _same_lists(got[0], corr)
    _same_lists(got[1], pc.pixels())
    # uint16, and the ROIs given as a mask stack
    uns = (raw.astype(np.int32) + 40000).astype(np.uint16)
    stack = np.zeros((len(rois), h, w), np.uint8)
    for n, r in enumerate(rois):
        stack[n, r[:, 0], r[:, 1]] = 1
    pu = RoiPairCorr((h, w), n_frames, uns.dtype, stack, chunk_frames=5).feed(uns)
    _check_against_reference(pu, uns, rois)


def test_shifts_and_fine_shifts_equal_the_recording_corrected_beforehand():
    from deep_calcium_amd import RoiPairCorr
    from test_footprints_gpu import _bilinear_host
    raw, rois = _recording()
    n_frames, h, w = raw.shape
    rs = np.random.RandomState(9)
    shifts = rs.randint(-3, 4, size=(n_frames, 2))
    moved = np.zeros_like(raw)
    for t, (dy, dx) in enumerate(shifts):
        ys, xs = np.arange(h) + dy, np.arange(w) + dx
        oky, okx = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
        moved[t][np.ix_(oky, okx)] = raw[t][np.ix_(ys[oky], xs[okx])]
    want = RoiPairCorr((h, w), n_frames, raw.dtype, rois).feed(moved)
    got = RoiPairCorr((h, w), n_frames, raw.dtype, rois, chunk_frames=5, shifts=shifts).feed(raw)
    _same_lists(got.result('corr'), want.result('corr'))
    assert np.array_equal(got.traces('sum'), want.traces('sum'))
    assert got.result('moments')[2]['g'].tolist() == want.result('moments')[2]['g'].tolist()
    _check_against_reference(got, moved, rois)
    fine = rs.randint(-40, 41, size=(n_frames, 2))
    fine[0] = (0, 0)
    fine[1] = (16, -32)
    interp = _bilinear_host(raw, fine)
    want = RoiPairCorr((h, w), n_frames, raw.dtype, rois).feed(interp)
    got = RoiPairCorr((h, w), n_frames, raw.dtype, rois, chunk_frames=5, fine_shifts=fine).feed(raw)
    assert np.array_equal(got.traces('sum'), want.traces('sum'))
    _same_lists(got.result('corr'), want.result('corr'))
    assert got.result('moments')[0]['a'].tolist() == want.result('moments')[0]['a'].tolist()


# ---- 4. the scene ------------------------------------------------------------------------------------------------------------
def test_the_scene_is_split_into_the_planted_halves(tmp_path):
    from deep_calcium_amd import RoiPairCorr, split_rois, split_rois_device
    frames, rois, left, right = ref.gpu_scene()
    n_frames, h, w = frames.shape
    path = str(tmp_path / 'scene.npz')
    np.savez(path, series_raw=frames)
    new, origin, gaps = split_rois_device(path, rois, min_gap=0.1, min_area=8, iterations=16, chunk_frames=100)
    assert origin == [0, 1, 1, 2, 3, 4] and len(new) == 6
    assert np.array_equal(new[1], left) and np.array_equal(new[2], right)           # 0 pixels misassigned, none dropped
    for n, r in ((0, 0), (3, 2), (4, 3), (5, 4)):
        assert new[n].dtype == np.int64 and np.array_equal(new[n], rois[r])         # the controls and the strip: unchanged
    assert gaps.dtype == np.float64 and gaps[1] >= 0.15 and np.isnan(gaps[2]) and all(not g >= 0.05 for g in gaps[[0, 3, 4]])
    # the same through the class (the strip's matrix is computed here, and passed over by the rule), and against the oracle
    pc = RoiPairCorr((h, w), n_frames, frames.dtype, rois, chunk_frames=100)
    for t0 in range(0, n_frames, 100):
        pc.feed(frames[t0:t0 + 100])
    corr = pc.result('corr')
    for r, c in enumerate(corr):
        assert np.abs(c.astype(np.float64) - ref.corrcoef(frames, rois[r])).max() < 1e-6
    again = split_rois(pc.pixels(), corr, (h, w), min_gap=0.1, min_area=8, iterations=16)
    assert again[1] == origin and all(np.array_equal(x, y) for x, y in zip(again[0], new))
    assert np.array_equal(again[2], gaps, equal_nan=True)
    want = ref.split(rois, corr, (h, w), min_gap=0.1, min_area=8, iterations=16)
    assert want[1] == origin and all(np.array_equal(x, y) for x, y in zip(want[0], new))
    # the same pass's traces
    assert np.array_equal(pc.traces('sum')[1], frames[:, rois[1][:, 0], rois[1][:, 1]].astype(np.int64).sum(1))
    # nothing is sent for ROIs beyond the limits: one of 1025 pixels comes back unchanged, without a pass
    path2 = str(tmp_path / 'flat.npz')
    np.savez(path2, series_raw=np.zeros((2, 33, 32), np.int16))
    huge = np.array([[y, x] for y in range(33) for x in range(32)])[:1025]
    new2, origin2, gaps2 = split_rois_device(path2, [huge, rois[2]], min_area=8)
    assert origin2 == [0, 1] and np.array_equal(new2[0], huge) and np.array_equal(new2[1], rois[2]) and np.isnan(gaps2).all()


def test_example_traces_command_splits_the_rois(tmp_path, monkeypatch, caplog):
    """examples/neurons/unet2ds_nf.py `traces --split GAP --min-area N`: the pair correlation, the split, then one trace per part.
    The prediction is stood in for by the scene's mask."""
    import importlib.util
    import logging
    import os
    from deep_calcium_amd import UNet2DSummary, hdf5_min
    frames, rois, left, right = ref.gpu_scene()
    n_frames, h, w = frames.shape
    mask2d = np.zeros((h, w), np.float32)
    for r in rois:
        mask2d[r[:, 0], r[:, 1]] = 0.9
    path = str(tmp_path / 'scene.npz')
    np.savez(path, series_raw=frames, series_mean=frames.mean(0).astype(np.float16), name=np.array('scene'))
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'neurons', 'unet2ds_nf.py')
    state = np.random.get_state()                             # the example seeds numpy's global stream on import
    try:
        spec = importlib.util.spec_from_file_location('example_unet2ds_nf_split', script)
        example = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(example)
    finally:
        np.random.set_state(state)
    monkeypatch.setattr(UNet2DSummary, 'predict', lambda self, dspaths, **kw: ([mask2d], ['scene']))
    cp = str(tmp_path / 'cp')
    with caplog.at_level(logging.INFO, logger='traces'):
        example.traces([path], None, cp, kind='sum', split=0.1, min_area=8)
    with hdf5_min.File(os.path.join(cp, 'scene_traces.hdf5')) as f:
        got = f['traces'].read()
    # the mask's regions in raster label order: the strip (row 0), then the four regions left to right
    assert got.dtype == np.int64 and got.shape == (6, n_frames)
    assert np.array_equal(got[2], frames[:, left[:, 0], left[:, 1]].astype(np.int64).sum(1))
    assert np.array_equal(got[3], frames[:, right[:, 0], right[:, 1]].astype(np.int64).sum(1))
    assert np.array_equal(got[0], frames[:, rois[2][:, 0], rois[2][:, 1]].astype(np.int64).sum(1))
    assert '1 of 5 ROIs split, 0 pixels dropped' in caplog.text
    # without the flag: one trace per region, as before
    cp2 = str(tmp_path / 'cp2')
    example.traces([path], None, cp2, kind='sum')
    with hdf5_min.File(os.path.join(cp2, 'scene_traces.hdf5')) as f:
        assert f['traces'].read().shape == (5, n_frames)
