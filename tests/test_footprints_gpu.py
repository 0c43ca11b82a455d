"""ROI footprint maps on the device (include/dcunet.h dc_roi_pixel_accumulate / dc_roi_trace_moments / dc_roi_pixel_corr;
deep_calcium_amd/footprints.py) against the Python-integer / 60-digit decimal reference of tests/_footprints_ref.py."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _footprints_ref as ref                     # noqa: E402
from test_series_gpu import _frames, _ulps        # noqa: E402  the full-range frames and the float32 distance of the series tests

SHAPES = [(1, 1), (5, 7), (33, 19), (16, 64)]
TS = [1, 3, 37]
M64 = (1 << 64) - 1


def _seg():
    from deep_calcium_amd.traces import SEGMENT_PIXELS
    return SEGMENT_PIXELS


def _i64(v):
    """The int64 that holds the low 64 bits of a Python int."""
    v &= M64
    return v - (1 << 64) if v >= (1 << 63) else v


def _layout(H, W):
    """-> (own, rows): the ROIs' own pixel lists (flat int32; what the sums are taken over) and the support rows (owner, flat
    indices) as the C ABI takes them: every length at which the kernel changes path, two rows that overlap, two that are
    identical, indices outside the image, and a row that names no ROI."""
    n = H * W
    rs = np.random.RandomState(11 * H + W)
    S = _seg()
    own = [np.array([n - 1]), np.array([0]),                                  # single pixels; _frames holds pixel 0 constant in time
           np.sort(rs.choice(n, min(n, 40), replace=False)), np.arange(n)]
    rows = []
    for j, k in enumerate((1, 63, 64, 65, S - 1, S, S + 1)):
        if k <= n:
            rows.append((j % 4, np.sort(rs.choice(n, k, replace=False))))
    rows.append((0, np.array([n - 1])))                                       # the own pixel of a one-pixel ROI
    rows.append((1, np.arange(0, min(n, 6))))                                 # the support of the constant trace
    rows.append((2, np.arange(0, min(n, 10))))                                # two that overlap
    rows.append((2, np.arange(min(n - 1, 5), min(n, 15))))
    same = np.sort(rs.choice(n, min(n, 20), replace=False))
    rows += [(3, same), (3, same.copy())]                                     # two identical
    rows.append((3, np.array([n, -1, 0, 2 ** 31 - 1, -2 ** 31, n // 2])))     # H*W, -1 and the int32 extremes contribute nothing
    rows.append((4, np.arange(0, min(n, 3))))                                 # names no ROI (R == 4): adds nothing
    rows.append((-1, np.arange(0, min(n, 3))))
    return [np.asarray(o, np.int32) for o in own], [(r, np.asarray(p, np.int32)) for r, p in rows]


class _Dev(object):
    """The raw C ABI on caller-owned buffers: what a binding without deep_calcium_amd/footprints.py would do."""

    def __init__(self, dclib, H, W, own, rows, T, pad=3):
        self.L, self.H, self.W, self.T, self.ld, self.R, self.S = dclib, H, W, T, T + pad, len(own), len(rows)
        cuda = lambda a, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dt))).cuda()      # noqa: E731
        self.own_off = cuda(np.concatenate([[0], np.cumsum([len(o) for o in own])]), np.int32)
        self.own_pix = cuda(np.concatenate(list(own) + [np.zeros(1, np.int32)]), np.int32)
        self.off = cuda(np.concatenate([[0], np.cumsum([len(p) for _, p in rows])]), np.int32)
        self.N = sum(len(p) for _, p in rows)
        self.pix = cuda(np.concatenate([p for _, p in rows] + [np.zeros(1, np.int32)]), np.int32)
        self.roi = cuda([r for r, _ in rows], np.int32)
        n = H * W
        flags = [np.isin(p, own[r]) if 0 <= r < len(own) else np.zeros(len(p), bool) for r, p in rows]
        self.inside_host = np.concatenate(flags) & (np.concatenate([p for _, p in rows]) < n) & (np.concatenate([p for _, p in rows]) >= 0)
        self.inside = cuda(self.inside_host, np.int32)
        self.sums = torch.full((self.R, self.ld), -0x0123456789abcdef, dtype=torch.int64, device='cuda')
        self.mom = torch.zeros((4, self.N), dtype=torch.int64, device='cuda')

    def _st(self):
        return torch.cuda.current_stream().cuda_stream

    def feed(self, dframes, uns, t0, tc, trace=True):
        fp = dframes[t0:t0 + tc].data_ptr()
        if trace:
            self.L.dc_roi_trace_accumulate(fp, uns, tc, t0, self.own_off.data_ptr(), self.own_pix.data_ptr(), None, self.R, self.R,
                                           self.sums.data_ptr(), self.ld, self.H, self.W, self._st())
        self.L.dc_roi_pixel_accumulate(fp, uns, tc, t0, self.off.data_ptr(), self.pix.data_ptr(), self.roi.data_ptr(), self.S, self.R,
                                       self.sums.data_ptr(), self.ld, self.mom.data_ptr(), self.N, self.H, self.W, self._st())

    def run(self, dframes, uns, chunks):
        self.mom.zero_()
        t0 = 0
        for tc in chunks:
            self.feed(dframes, uns, t0, tc)
            t0 += tc
        assert t0 == self.T
        torch.cuda.synchronize()
        return self.mom.cpu().numpy()

    def corr(self):
        rmom = torch.full((3, self.R), 77, dtype=torch.int64, device='cuda')
        out = torch.full((self.N + 2,), float('nan'), dtype=torch.float32, device='cuda')
        self.L.dc_roi_trace_moments(self.sums.data_ptr(), self.ld, self.R, self.T, rmom.data_ptr(), self._st())
        self.L.dc_roi_pixel_corr(self.mom.data_ptr(), self.N, self.off.data_ptr(), self.roi.data_ptr(), self.S, self.R,
                                 self.inside.data_ptr(), rmom.data_ptr(), self.T, out.data_ptr(), self._st())
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert np.isnan(out[self.N:]).all()              # nothing beyond the N entries is written
        return rmom.cpu().numpy(), out[:self.N]


def _device_frames(frames):
    return torch.from_numpy(np.ascontiguousarray(frames).view(np.int16)).cuda()


@functools.lru_cache(maxsize=None)
def _case(shape, T, dtype_name, seed=0):
    """Frames, layout and the Python-integer reference of one case, computed once and shared: per row the list of (a, b, c), per
    ROI the trace S."""
    H, W = shape
    dtype = np.dtype(dtype_name).type
    frames = _frames(T, H, W, dtype, seed=seed)
    own, rows = _layout(H, W)
    S = [ref.sums(frames, [int(p) for p in o]) for o in own]
    mom = []
    for r, p in rows:
        if 0 <= r < len(own):
            mom += ref.moments(frames, [int(q) for q in p], S[r])
        else:
            mom += [(0, 0, 0)] * len(p)
    return frames, own, rows, S, mom


def _planes(mom):
    return np.array([[a for a, _, _ in mom], [b for _, b, _ in mom], [_i64(c) for _, _, c in mom], [c >> 64 for _, _, c in mom]], np.int64)


def _chunkings(T):
    out = [[T]]
    if T > 1:
        out += [[1] * T, [T // 3 + 1, T - (T // 3 + 1)] if T < 10 else [5, 1, T - 22, 16]]
    return out


# ---- 1. the raw ABI: moments exact ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.int16, np.uint16], ids=['int16', 'uint16'])
@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%d' % s for s in SHAPES])
def test_moments_equal_python_integers_for_every_chunking(dclib, shape, dtype):
    H, W = shape
    lengths = set()
    for T in TS:
        frames, own, rows, S, mom = _case(shape, T, np.dtype(dtype).name)
        lengths |= set(len(p) for _, p in rows)
        want = _planes(mom)
        dframes = _device_frames(frames)
        first = None
        for chunks in _chunkings(T) + [[T]]:                 # the last: a second run of the first
            st = _Dev(dclib, H, W, own, rows, T)
            got = st.run(dframes, int(dtype == np.uint16), chunks)
            for k, name in enumerate(('a', 'b', 'c_lo', 'c_hi')):
                assert np.array_equal(got[k], want[k]), (T, chunks, name)
            first = got if first is None else first
            assert np.array_equal(first, got)
        assert np.array_equal(st.sums.cpu().numpy()[:, :T], np.array(S, np.int64))
    if H * W >= _seg() + 1:
        assert lengths >= {1, 63, 64, 65, _seg() - 1, _seg(), _seg() + 1}


def test_moments_across_the_staging_boundary(dclib):
    """T = 1030 in one launch: two full stages of the ROI's trace in LDS and a tail of 6 frames (no multiple of the frames in
    flight), against chunks that end on, before and after the boundary."""
    H, W, T = 5, 7, 1030
    frames = _frames(T, H, W, np.int16, seed=3)
    own, rows = _layout(H, W)
    S = [ref.sums(frames, [int(p) for p in o]) for o in own]
    mom = []
    for r, p in rows:
        mom += ref.moments(frames, [int(q) for q in p], S[r]) if 0 <= r < len(own) else [(0, 0, 0)] * len(p)
    want = _planes(mom)
    dframes = _device_frames(frames)
    for chunks in ([T], [512, 518], [511, 2, 517], [1024, 6]):
        got = _Dev(dclib, H, W, own, rows, T).run(dframes, 0, chunks)
        assert np.array_equal(got, want), chunks


# ---- 2. fabricated sums ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.int16, np.uint16], ids=['int16', 'uint16'])
def test_products_with_sums_of_46_bits_are_exact(dclib, dtype):
    """sums written by the test: +-2^46 and mixed signs, against pixels at the types' extremes, 37 frames in one launch.
    65535 * 2^46 * 37 > 2^67: a running int64 sum of the products wraps."""
    H, W, T = 5, 7, 37
    info = np.iinfo(dtype)
    rs = np.random.RandomState(8)
    frames = rs.choice([info.min, info.max], size=(T, H, W)).astype(dtype)
    frames[:, 0, 0] = info.max
    frames[:, 0, 1] = info.min
    frames[:, 0, 2] = rs.randint(info.min, info.max + 1, size=T)
    own = [np.array([0], np.int32)] * 4
    every = np.arange(H * W, dtype=np.int32)
    rows = [(r, every) for r in range(4)]
    S = [[2 ** 46] * T, [-2 ** 46] * T, [int(v) for v in rs.choice([2 ** 46, -2 ** 46, 2 ** 46 - 1, 1 - 2 ** 46, 2 ** 32, -1], size=T)],
         [int(v) for v in rs.randint(-2 ** 46, 2 ** 46 + 1, size=T)]]
    st = _Dev(dclib, H, W, own, rows, T)
    st.sums[:, :T] = torch.from_numpy(np.array(S, np.int64)).cuda()
    st.feed(_device_frames(frames), int(dtype == np.uint16), 0, T, trace=False)
    torch.cuda.synchronize()
    got = st.mom.cpu().numpy()
    mom = []
    for r, p in rows:
        mom += ref.moments(frames, [int(q) for q in p], S[r])
    assert max(abs(c) for _, _, c in mom) > 2 ** 66
    assert np.array_equal(got, _planes(mom))


# ---- 3. corr ---------------------------------------------------------------------------------------------------------------
def _corr_ref(T, rows, own, S, mom, inside):
    exact, plain = [], []
    e = 0
    for r, p in rows:
        for _ in p:
            if 0 <= r < len(own):
                u, w = sum(S[r]), sum(s * s for s in S[r])
                a, b, c = mom[e]
                exact.append(ref.corr_exact(T, a, b, c, u, w, bool(inside[e])))
                plain.append(ref.corr(T, a, b, c, u, w, bool(inside[e])))
            else:
                exact.append(np.float32(0)); plain.append(np.float32(0))
            e += 1
    return np.array(exact, np.float32), np.array(plain, np.float32)


@pytest.mark.parametrize('dtype', [np.int16, np.uint16], ids=['int16', 'uint16'])
@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%d' % s for s in SHAPES])
def test_corr_is_within_one_ulp_of_exact_arithmetic(dclib, shape, dtype):
    H, W = shape
    for T in TS:
        frames, own, rows, S, mom = _case(shape, T, np.dtype(dtype).name)
        st = _Dev(dclib, H, W, own, rows, T)
        st.run(_device_frames(frames), int(dtype == np.uint16), [T])
        rmom, got = st.corr()
        for r in range(len(own)):
            u, w = sum(S[r]), sum(s * s for s in S[r])
            assert [int(v) for v in rmom[:, r]] == [u, _i64(w), w >> 64], (T, r)
        exact, plain = _corr_ref(T, rows, own, S, mom, st.inside_host)
        assert np.isfinite(got).all()
        d = _ulps(got, exact)
        print('corr %r T=%d %s: max %d ulp of exact, %d of the double formula' % (shape, T, np.dtype(dtype).name, d.max(), _ulps(got, plain).max()))
        assert d.max() <= 1, (T, int(d.max()))
        assert np.abs(got).max() <= 1.0
        # exactly 0: T == 1, a constant pixel (the first 4 or 5 of _frames hold one value each), a constant trace (ROI 1 is pixel
        # 0), the pixel of a one-pixel ROI, an index outside the image, a row that names no ROI
        still = 0 if H * W == 1 else (5 if dtype == np.uint16 else 4)
        e, zero = 0, np.zeros(len(got), bool)
        for r, p in rows:
            for q in p:
                inside = bool(st.inside_host[e])
                zero[e] = (T == 1 or r in (1, 4, -1) or not still <= q < H * W or (inside and len(own[r]) == 1))
                e += 1
        assert not got[zero].any() and not np.signbit(got[zero]).any(), T
        if T > 1 and H * W > 40:
            assert (got[~zero] != 0).all()


def test_corr_of_equal_and_mirrored_series_is_plus_and_minus_one(dclib):
    H, W, T = 5, 7, 37
    frames = _frames(T, H, W, np.int16, seed=2) // 4
    p, q, m, k = 17, 30, 9, 20
    frames.reshape(T, -1)[:, q] = frames.reshape(T, -1)[:, p]                 # equal to the one-pixel ROI's trace
    frames.reshape(T, -1)[:, m] = 1234 - frames.reshape(T, -1)[:, p]          # mirrored about a constant
    frames.reshape(T, -1)[:, k] = -77                                         # constant
    own = [np.array([p], np.int32), np.array([k], np.int32)]
    rows = [(0, np.array([m, p, k, q, 12], np.int32)), (1, np.array([k, p, q], np.int32))]
    st = _Dev(dclib, H, W, own, rows, T)
    st.run(_device_frames(frames), 0, [20, 17])
    _, got = st.corr()
    assert got[:4].tolist() == [-1.0, 0.0, 0.0, 1.0] and 0 < abs(got[4]) < 1
    assert got[5:].tolist() == [0.0, 0.0, 0.0]                                # a constant trace
    # a pair of pixels: each is the other's leave-one-out trace
    own = [np.array([p, q], np.int32), np.array([p, m], np.int32)]
    rows = [(0, np.array([p, q], np.int32)), (1, np.array([m, p], np.int32))]
    st = _Dev(dclib, H, W, own, rows, T)
    st.run(_device_frames(frames), 0, [T])
    assert st.corr()[1].tolist() == [1.0, 1.0, -1.0, -1.0]


# ---- 4. the Python API -------------------------------------------------------------------------------------------------------
def _same_lists(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert np.array_equal(x.view(np.int32) if x.dtype == np.float32 else x, y.view(np.int32) if y.dtype == np.float32 else y)


def _recording():
    rs = np.random.RandomState(6)
    T, H, W = 12, 24, 24
    raw = rs.randint(-300, 3000, size=(T, H, W)).astype(np.int16)
    rois = [np.argwhere(np.pad(np.ones((4, 5), bool), ((3, 17), (2, 17)))), np.array([[0, 0], [0, 1], [1, 0]]),
            np.argwhere(np.pad(np.ones((5, 4), bool), ((5, 14), (5, 15)))), np.array([[23, 23]])]
    for r in rois[:3]:
        raw[:, r[:, 0], r[:, 1]] += rs.randint(0, 2000, size=(T, 1)).astype(np.int16)
    return raw, rois


def _check_against_reference(fp, frames, rois, halo):
    H, W = frames.shape[1:]
    coords, inside = ref.support(rois, (H, W), halo)
    _same_lists(fp.support(), coords)
    _same_lists(fp.inside(), inside)
    m = ref.maps(frames, coords, inside, rois)
    got_m, got_c = fp.result('moments'), fp.result('corr')
    for r in range(len(rois)):
        assert got_m[r]['a'].dtype == object
        assert [(int(a), int(b), int(c)) for a, b, c in zip(got_m[r]['a'], got_m[r]['b'], got_m[r]['c'])] == m[r][0], r
        assert got_c[r].dtype == np.float32 and _ulps(got_c[r], m[r][2]).max() <= 1, r
    coh = fp.result('coherence')
    assert coh.dtype == np.float64 and coh.shape == (len(rois),)
    assert np.array_equal(coh, np.array([c[i].astype(np.float64).mean() for c, i in zip(got_c, inside)]))
    return got_c


def test_class_numpy_chunks_resident_tensor_and_file_agree(tmp_path):
    from deep_calcium_amd import RoiFootprints, RoiTraceExtractor, roi_footprints_device
    raw, rois = _recording()
    T, H, W = raw.shape
    fp = RoiFootprints((H, W), T, raw.dtype, rois, halo=2, chunk_frames=5)
    assert fp.feed(raw[:7]) is fp
    fp.feed(raw[7:])
    corr = _check_against_reference(fp, raw, rois, 2)
    assert corr[3][fp.inside()[3]].tolist() == [0.0]                          # the pixel of a one-pixel ROI
    ext = RoiTraceExtractor((H, W), T, raw.dtype, rois).feed(raw)
    assert np.array_equal(fp.traces('sum'), ext.result('sum'))
    assert np.array_equal(fp.traces('zscore').view(np.int32), ext.result('zscore').view(np.int32))
    assert ext._stage._host[0] is not fp._ext._stage._host[0]                 # staging slots of its own
    res = RoiFootprints((H, W), T, raw.dtype, rois, halo=2)
    with pytest.raises(ValueError, match='after 0 of 12'):
        res.result('corr')
    res.feed(torch.from_numpy(raw).cuda())
    with pytest.raises(ValueError, match='not one of'):
        res.result('median')
    _same_lists(res.result('corr'), corr)
    assert res.result('moments')[0]['c'].tolist() == fp.result('moments')[0]['c'].tolist()
    path = str(tmp_path / 'rec.npz')
    np.savez(path, series_raw=raw)
    got = roi_footprints_device(path, rois, halo=2, chunk_frames=4)
    _same_lists(got[0], corr)
    _same_lists(got[1], fp.support())
    _same_lists(got[2], fp.inside())
    # uint16, halo 0: every entry is inside
    uns = (raw.astype(np.int32) + 40000).astype(np.uint16)
    fu = RoiFootprints((H, W), T, uns.dtype, rois, halo=0, chunk_frames=5).feed(uns)
    _check_against_reference(fu, uns, rois, 0)
    assert all(i.all() for i in fu.inside())


def _bilinear_host(raw, fine):
    """The README's formula for fine (sixteenths of a pixel) rigid shifts, fill 0: out = (sum of the four neighbours weighted by
    (16 - fy)(16 - fx), ... + 128) >> 8 in integers, 0 where a neighbour lies outside the frame."""
    T, H, W = raw.shape
    out = np.zeros_like(raw)
    for t in range(T):
        dy, dx = int(fine[t, 0]), int(fine[t, 1])
        iy, fy, ix, fx = dy >> 4, dy & 15, dx >> 4, dx & 15
        for y in range(H):
            for x in range(W):
                y0, x0 = y + iy, x + ix
                y1, x1 = y0 + (1 if fy else 0), x0 + (1 if fx else 0)
                if y0 < 0 or x0 < 0 or y1 >= H or x1 >= W:
                    continue
                f = raw[t].astype(np.int64)
                v = (16 - fy) * (16 - fx) * f[y0, x0] + (16 - fy) * fx * f[y0, x1] + fy * (16 - fx) * f[y1, x0] + fy * fx * f[y1, x1]
                out[t, y, x] = (v + 128) >> 8
    return out


def test_shifts_and_fine_shifts_equal_the_recording_corrected_beforehand():
    from deep_calcium_amd import RoiFootprints
    raw, rois = _recording()
    T, H, W = raw.shape
    rs = np.random.RandomState(9)
    shifts = rs.randint(-3, 4, size=(T, 2))
    moved = np.zeros_like(raw)
    for t, (dy, dx) in enumerate(shifts):
        ys, xs = np.arange(H) + dy, np.arange(W) + dx
        oky, okx = (ys >= 0) & (ys < H), (xs >= 0) & (xs < W)
        moved[t][np.ix_(oky, okx)] = raw[t][np.ix_(ys[oky], xs[okx])]
    want = RoiFootprints((H, W), T, raw.dtype, rois, halo=2).feed(moved)
    got = RoiFootprints((H, W), T, raw.dtype, rois, halo=2, chunk_frames=5, shifts=shifts).feed(raw)
    _same_lists(got.result('corr'), want.result('corr'))
    assert np.array_equal(got.traces('sum'), want.traces('sum'))
    assert got.result('moments')[0]['c'].tolist() == want.result('moments')[0]['c'].tolist()
    _check_against_reference(got, moved, rois, 2)
    fine = rs.randint(-40, 41, size=(T, 2))
    fine[0] = (0, 0)
    fine[1] = (16, -32)
    interp = _bilinear_host(raw, fine)
    want = RoiFootprints((H, W), T, raw.dtype, rois, halo=2).feed(interp)
    got = RoiFootprints((H, W), T, raw.dtype, rois, halo=2, chunk_frames=5, fine_shifts=fine).feed(raw)
    assert np.array_equal(got.traces('sum'), want.traces('sum'))
    _same_lists(got.result('corr'), want.result('corr'))


# ---- 5. a synthetic scene ----------------------------------------------------------------------------------------------------
def test_the_scene_is_refined_to_the_true_cell():
    from deep_calcium_amd import RoiFootprints, refine_rois
    frames, rois, cell, blob = ref.scene()
    T, H, W = frames.shape
    fp = RoiFootprints((H, W), T, frames.dtype, rois, halo=2, chunk_frames=150)
    for a in range(0, T, 150):
        fp.feed(frames[a:a + 150])
    coords, inside, corr = fp.support(), fp.inside(), fp.result('corr')
    want_c, want_i = ref.support(rois, (H, W), 2)
    _same_lists(coords, want_c)
    m = ref.maps(frames, want_c, want_i, rois)
    for r in range(2):
        assert _ulps(corr[r], m[r][2]).max() <= 1
    cell_set = set(map(tuple, cell.tolist()))
    true = np.array([tuple(p) in cell_set for p in coords[0].tolist()])
    assert corr[0][true].min() > 0.5 and np.abs(corr[0][~true]).max() < 0.2 and np.abs(corr[1]).max() < 0.2
    assert fp.result('coherence')[1] < 0.1 and fp.result('coherence')[0] > 0.3
    new, kept = refine_rois(coords, corr, (H, W), threshold=0.3)
    assert kept == [0] and len(new) == 1 and np.array_equal(new[0], cell)      # exactly the true cell; the blob is dropped
    want_new, want_kept = ref.refine(want_c, [x[1] for x in m], (H, W), 0.3)
    assert kept == want_kept and np.array_equal(new[0], want_new[0])


def test_example_traces_command_refines_the_rois_first(tmp_path, monkeypatch, caplog):
    """examples/neurons/unet2ds_nf.py `traces --refine THR --halo N`: maps, refinement, then the traces of the refined ROIs.  The
    prediction is stood in for by the scene's mask (the cell and the blob, each a pixel too fat)."""
    import importlib.util
    import logging
    import os
    from deep_calcium_amd import UNet2DSummary, hdf5_min
    frames, rois, cell, blob = ref.scene()
    T, H, W = frames.shape
    mask2d = np.zeros((H, W), np.float32)
    for r in rois:
        mask2d[r[:, 0], r[:, 1]] = 0.9
    path = str(tmp_path / 'scene.npz')
    np.savez(path, series_raw=frames, series_mean=frames.mean(0).astype(np.float16), name=np.array('scene'))
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'neurons', 'unet2ds_nf.py')
    state = np.random.get_state()                             # the example seeds numpy's global stream on import
    try:
        spec = importlib.util.spec_from_file_location('example_unet2ds_nf_refine', script)
        example = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(example)
    finally:
        np.random.set_state(state)
    monkeypatch.setattr(UNet2DSummary, 'predict', lambda self, dspaths, **kw: ([mask2d], ['scene']))
    cp = str(tmp_path / 'cp')
    with caplog.at_level(logging.INFO, logger='traces'):
        example.traces([path], None, cp, kind='sum', refine=0.3, halo=2)
    with hdf5_min.File(os.path.join(cp, 'scene_traces.hdf5')) as f:
        got = f['traces'].read()
    assert got.dtype == np.int64 and got.shape == (1, T)
    assert np.array_equal(got[0], frames[:, cell[:, 0], cell[:, 1]].astype(np.int64).sum(1))
    removed = sum(len(r) for r in rois) - len(cell)
    assert '1 of 2 ROIs dropped, %d pixels removed, 0 added' % removed in caplog.text
