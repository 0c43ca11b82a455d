"""Device-side series summaries (include/dcunet.h dc_series_*, dc_image_standardize; deep_calcium_amd/series.py) against the
reference's own output, numpy integers and float64 / exact-integer references computed here."""
import decimal
import functools
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

SHAPES = [(1, 1), (1, 9), (5, 7), (33, 19), (16, 64)]
TS = [1, 2, 3, 37]


def _frames(T, H, W, dtype, seed=0):
    """Full-range random frames whose first pixels walk through the type's extremes (int16: -32768, 32767; uint16: 0, 32768,
    65535), held for all frames or alternating between them."""
    rs = np.random.RandomState(1000 * T + 10 * H + W + seed)
    info = np.iinfo(dtype)
    f = rs.randint(info.min, info.max + 1, size=(T, H * W)).astype(dtype)
    special = [info.min, info.max] + ([32768, 0, 65535] if dtype == np.uint16 else [-1, 0])
    for j in range(min(H * W, 2 * len(special))):
        for t in range(T):
            f[t, j] = special[(j + (t if j >= len(special) or H * W == 1 else 0)) % len(special)]
    return f.reshape(T, H, W)


class _State(object):
    """The raw C ABI on caller-owned buffers: what a binding without deep_calcium_amd/series.py would do."""

    def __init__(self, dclib, H, W, chain=True, xy=True):
        n = H * W
        dev = 'cuda'
        self.L, self.H, self.W = dclib, H, W
        # filled with garbage on purpose: the chunk with t0 == 0 must initialise every buffer
        self.sum = torch.full((n,), -77, dtype=torch.int64, device=dev)
        self.sumsq = torch.full((n,), 99, dtype=torch.int64, device=dev)
        self.vmax = torch.full((n,), 123456, dtype=torch.int32, device=dev)
        self.mean16 = torch.full((n,), 0x7e00, dtype=torch.int16, device=dev) if chain else None
        self.max16 = torch.full((n,), 31000, dtype=torch.int16, device=dev) if chain else None
        self.xy = torch.full((4, n), 5, dtype=torch.int64, device=dev) if xy else None

    def run(self, frames, chunk):
        T = frames.shape[0]
        uns = int(frames.dtype == np.uint16)
        st = torch.cuda.current_stream().cuda_stream
        keep = []
        for t0 in range(0, T, chunk):
            part = np.ascontiguousarray(frames[t0:t0 + chunk]).view(np.int16)
            d = torch.from_numpy(part).cuda()
            keep.append(d)
            self.L.dc_series_accumulate(d.data_ptr(), uns, part.shape[0], t0, T,
                                        self.mean16.data_ptr() if self.mean16 is not None else None,
                                        self.max16.data_ptr() if self.max16 is not None else None,
                                        self.sum.data_ptr(), self.sumsq.data_ptr(), self.vmax.data_ptr(), self.H, self.W, st)
            if self.xy is not None:
                self.L.dc_series_accumulate_xy(d.data_ptr(), uns, part.shape[0], t0, self.xy.data_ptr(), self.H, self.W, st)
        torch.cuda.synchronize()
        return self

    def finalize(self, T, corr=True):
        out = torch.full((3, self.H * self.W), float('nan'), dtype=torch.float32, device='cuda')
        self.L.dc_series_finalize(self.sum.data_ptr(), self.sumsq.data_ptr(), self.xy.data_ptr() if corr else None,
                                  out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr() if corr else None,
                                  self.H, self.W, T, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return [o.reshape(self.H, self.W) for o in out.cpu().numpy()]


def _xy_ref(x):
    """int64 cross sums with the right, down, down-right and down-left neighbour; 0 where there is none."""
    T, H, W = x.shape
    out = np.zeros((4, H, W), np.int64)
    out[0, :, :W - 1] = (x[:, :, :-1] * x[:, :, 1:]).sum(0)
    out[1, :H - 1, :] = (x[:, :-1, :] * x[:, 1:, :]).sum(0)
    out[2, :H - 1, :W - 1] = (x[:, :-1, :-1] * x[:, 1:, 1:]).sum(0)
    out[3, :H - 1, 1:] = (x[:, :-1, 1:] * x[:, 1:, :-1]).sum(0)
    return out


def _mean16_ref(frames):
    """datasets/nf.py:129 as nf_datasets._populate runs it."""
    n = frames.shape[0]
    mean = np.zeros(frames.shape[1:], np.float16)
    with np.errstate(over='ignore'):
        for img in frames:
            mean = (mean + (img * 1. / n)).astype(np.float16)
    return mean


def _max16_ref(frames):
    mx = np.zeros(frames.shape[1:], np.int64)
    for img in frames:
        mx = np.minimum(np.maximum(mx, img.astype(np.int64)), 32767)
    return mx.astype(np.int16)


def _ulps(a, b):
    """distance in float32 steps (+0 == -0); both finite"""
    def key(v):
        i = np.ascontiguousarray(v, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


# ---- 1. the reference's own output ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['neurofinder.00.00', 'neurofinder.01.00.test'])
def test_stored_mean_and_max_equal_the_references_dataset_file(golden_dir, name):
    """tests/golden/nf_dataset.npz: nf_load_hdf5 of the reference run with real h5py.  Chunks of 4 divide neither 9 nor 5."""
    import os
    from deep_calcium_amd import SeriesSummarizer
    z = np.load(os.path.join(golden_dir, 'nf_dataset.npz'))
    frames = z['frames_' + name]
    T, H, W = frames.shape
    s = SeriesSummarizer((H, W), T, frames.dtype, chunk_frames=4, kinds=('mean16', 'max16'))
    s.feed(frames[:3]).feed(frames[3:])          # chunks of 3, then 4 + 2 (or 2): feed() cuts what exceeds chunk_frames itself
    want = z[name + ':series/mean']
    got = s.result('mean16')
    assert got.dtype == np.float16 and want.dtype == np.float16
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))
    if name == 'neurofinder.00.00':
        assert np.isinf(want).any()            # the pixel that overflows float16 is in the fixture
    got = s.result('max16')
    assert got.dtype == np.int16 and np.array_equal(got, z[name + ':series/max'])


# ---- 2. + 3. exact state and the float16 chain ------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', [np.int16, np.uint16], ids=['int16', 'uint16'])
@pytest.mark.parametrize('shape', SHAPES, ids=['%dx%d' % s for s in SHAPES])
def test_integer_state_and_float16_chain_equal_numpy_for_every_chunking(dclib, shape, dtype):
    H, W = shape
    for T in TS:
        frames = _frames(T, H, W, dtype)
        x = frames.astype(np.int64)
        want = dict(sum=x.sum(0), sumsq=(x * x).sum(0), vmax=x.max(0), xy=_xy_ref(x),
                    mean16=_mean16_ref(frames).view(np.uint16), max16=_max16_ref(frames))
        assert H * W == 1 or set(frames.ravel().tolist()) >= {np.iinfo(dtype).min, np.iinfo(dtype).max}
        for chunk in sorted({1, 2, 16, T}):
            s = _State(dclib, H, W).run(frames, chunk)
            tag = (T, chunk)
            assert np.array_equal(s.sum.cpu().numpy().reshape(H, W), want['sum']), tag
            assert np.array_equal(s.sumsq.cpu().numpy().reshape(H, W), want['sumsq']), tag
            assert np.array_equal(s.vmax.cpu().numpy().reshape(H, W), want['vmax']), tag
            assert np.array_equal(s.xy.cpu().numpy().reshape(4, H, W), want['xy']), tag
            assert np.array_equal(s.mean16.cpu().numpy().view(np.uint16).reshape(H, W), want['mean16']), tag
            assert np.array_equal(s.max16.cpu().numpy().reshape(H, W), want['max16']), tag


def test_float16_chain_when_increments_fall_below_half_an_ulp(dclib):
    """300 frames of a constant 1000 (every increment of 3.33 is rounded to a float16 spacing of up to 0.5, so the chain ends
    at 1019, not 1000), of 30 and of -7, and a pixel that holds 32767 for 150 frames and 1 afterwards: its mean sits near
    16384, where float16 steps by 16, and the increments of 1/300 vanish entirely."""
    T, H, W = 300, 5, 7
    frames = np.full((T, H, W), 1000, np.int16)
    frames[:, 2, 3] = 30
    frames[:, 4, 6] = -7
    frames[:150, 1, 1], frames[150:, 1, 1] = 32767, 1
    want = _mean16_ref(frames)
    assert want[0, 0] == np.float16(1019) and want[2, 3] != np.float16(30)      # the chain is NOT the mean rounded once
    assert want[1, 1] == np.float16(16540)                                      # stalled: the true mean is 16384
    for chunk in (16, 7, 300):
        s = _State(dclib, H, W, xy=False).run(frames, chunk)
        assert np.array_equal(s.mean16.cpu().numpy().view(np.uint16).reshape(H, W), want.view(np.uint16)), chunk


# ---- 4. mean / std / corr ------------------------------------------------------------------------------------------------
def _moments_ref(frames):
    """(mean, std, corr) as float32 images: exact Python-integer numerators, 60-digit decimal division / square root, one
    rounding at the end (decimal -> double -> float32; the double step moves the result by < 2^-29 float32 ulp)."""
    T, H, W = frames.shape
    ctx = decimal.Context(prec=60)
    x = frames.astype(object)                      # Python integers
    sx = x.sum(0)
    sxx = (x * x).sum(0)
    var = T * sxx - sx * sx                        # exact, >= 0
    mean = np.array([[float(ctx.divide(decimal.Decimal(int(v)), decimal.Decimal(T))) for v in row] for row in sx], np.float64)
    std = np.array([[float(ctx.divide(ctx.sqrt(decimal.Decimal(int(v))), decimal.Decimal(T))) for v in row] for row in var], np.float64)
    corr = np.zeros((H, W), np.float64)
    for y, xx in itertools.product(range(H), range(W)):
        acc, cnt = decimal.Decimal(0), 0
        for dy, dx in itertools.product((-1, 0, 1), (-1, 0, 1)):
            qy, qx = y + dy, xx + dx
            if (dy, dx) == (0, 0) or not (0 <= qy < H and 0 <= qx < W):
                continue
            cnt += 1
            vp, vq = int(var[y, xx]), int(var[qy, qx])
            if vp == 0 or vq == 0:
                continue
            num = T * int((x[:, y, xx] * x[:, qy, qx]).sum()) - int(sx[y, xx]) * int(sx[qy, qx])
            acc = ctx.add(acc, ctx.divide(decimal.Decimal(num), ctx.sqrt(decimal.Decimal(vp * vq))))
        corr[y, xx] = float(ctx.divide(acc, decimal.Decimal(cnt))) if cnt else 0.0
    return mean.astype(np.float32), std.astype(np.float32), corr.astype(np.float32)


def _structured(T, H, W, dtype):
    """Random frames with spatial correlation (a shared signal), a constant pixel, and a varying pixel inside a 3x3 block of
    constants."""
    rs = np.random.RandomState(5 + T + H)
    info = np.iinfo(dtype)
    base = rs.randint(-3000, 3000, size=(T, 1, 1))
    f = base * rs.uniform(-1, 1, size=(1, H, W)) + rs.randint(-2000, 2000, size=(T, H, W)) + (info.max + info.min + 1) // 2
    f = np.clip(np.rint(f), info.min, info.max).astype(dtype)
    if H >= 5 and W >= 5:
        f[:, 0, 2] = info.max                                   # a constant pixel among varying ones
        centre = f[:, 3, 3].copy()
        f[:, 2:5, 2:5] = np.arange(9).reshape(3, 3) + 100       # constants (in time), all different
        f[:, 3, 3] = centre                                     # ... around a pixel that varies
    return f


@pytest.mark.parametrize('dtype', [np.int16, np.uint16], ids=['int16', 'uint16'])
@pytest.mark.parametrize('shape', [(1, 1), (1, 9), (5, 7), (33, 19)], ids=['1x1', '1x9', '5x7', '33x19'])
def test_mean_std_corr_within_one_ulp_of_exact_arithmetic(dclib, shape, dtype):
    H, W = shape
    for T, chunk in ((1, 1), (3, 2), (37, 16)):
        for frames in (_structured(T, H, W, dtype), _frames(T, H, W, dtype, seed=1)):
            mean, std, corr = _State(dclib, H, W, chain=False).run(frames, chunk).finalize(T)
            rmean, rstd, rcorr = _moments_ref(frames)
            for name, got, want in (('mean', mean, rmean), ('std', std, rstd), ('corr', corr, rcorr)):
                assert np.isfinite(got).all(), name
                d = _ulps(got, want)
                print('%s %dx%d T=%d %s: max %d ulp' % (name, H, W, T, np.dtype(dtype).name, d.max()))
                assert d.max() <= 1, (name, T, int(d.max()))
            assert np.abs(corr).max() <= 1.0
            if T == 1:
                assert not std.any()                 # one frame: no variance (a 1x1 image of several frames has one)
            if T == 1 or H * W == 1:
                assert not corr.any()                # no variance, or no neighbour
            if H >= 5 and W >= 5 and T > 1 and frames[0, 2, 2] == 100:
                assert corr[0, 2] == 0.0 and std[0, 2] == 0.0        # the constant pixel
                assert corr[3, 3] == 0.0 and std[3, 3] > 0.0         # varies, but every neighbour is constant
                assert not corr[2:5, 2:5].any()


def test_corr_is_exactly_zero_or_plus_minus_one_where_it_has_to_be(dclib):
    """Zero: a pixel without neighbours; a 1xN image whose pixels are constant in time (different from each other); an image
    whose values are all equal.  (A 1xN image of VARYING pixels has left / right neighbours and a correlation like any other:
    test_mean_std_corr_within_one_ulp_of_exact_arithmetic covers 1x9.)  One: two pixels with the same series; minus one: x and c - x."""
    T = 20
    rs = np.random.RandomState(11)
    run = lambda f: _State(dclib, f.shape[1], f.shape[2], chain=False).run(f, 7).finalize(f.shape[0])
    _, std, corr = run(rs.randint(-32768, 32768, size=(T, 1, 1)).astype(np.int16))
    assert corr[0, 0] == 0.0 and std[0, 0] > 0
    _, std, corr = run(np.broadcast_to(np.arange(9, dtype=np.int16) * 3000 - 9000, (T, 1, 9)).copy())
    assert not corr.any() and not std.any()
    for v, dtype in ((-32768, np.int16), (65535, np.uint16), (0, np.int16)):
        mean, std, corr = run(np.full((T, 4, 6), v, dtype))
        assert not corr.any() and not std.any() and (mean == v).all()
    x = rs.randint(0, 65536, size=T).astype(np.uint16)
    f = np.stack([x, x], 1).reshape(T, 1, 2)
    assert np.array_equal(run(f)[2], np.ones((1, 2), np.float32))
    assert np.array_equal(run(f.reshape(T, 2, 1))[2], np.ones((2, 1), np.float32))
    f = np.stack([x, 65535 - x], 1).reshape(T, 1, 2)
    assert np.array_equal(run(f)[2], -np.ones((1, 2), np.float32))
    # diagonal neighbours only: identical on one diagonal, opposite on the other, constants elsewhere
    f = np.zeros((T, 2, 2), np.uint16)
    f[:, 0, 0], f[:, 1, 1] = x, x
    assert np.array_equal(run(f)[2], np.array([[1, 0], [0, 1]], np.float32) / 3)
    f[:, 0, 0], f[:, 1, 1] = 7, 9
    f[:, 0, 1], f[:, 1, 0] = x, 65535 - x
    assert np.array_equal(run(f)[2], np.array([[0, -1], [-1, 0]], np.float32) / 3)


# ---- 5. standardisation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(5, 7), (33, 19)], ids=['5x7', '33x19'])
def test_image_standardize_within_one_ulp_of_float64(dclib, shape):
    H, W = shape
    rs = np.random.RandomState(H)
    img = (rs.random_sample(shape) * 900 + 50).astype(np.float16).astype(np.float32)      # what series/mean looks like
    s64 = img.astype(np.float64)
    want = ((s64 - s64.mean()) / s64.std()).astype(np.float32)
    src = torch.from_numpy(img).cuda()
    out = torch.empty_like(src)
    ws = torch.empty(dclib.dc_series_standardize_ws_floats(H, W), dtype=torch.float32, device='cuda')
    dclib.dc_image_standardize(src.data_ptr(), out.data_ptr(), ws.data_ptr(), H, W, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    d = _ulps(out.cpu().numpy(), want)
    print('standardize %dx%d: max %d ulp' % (H, W, d.max()))
    assert d.max() <= 1
    assert np.array_equal(src.cpu().numpy(), img)


# ---- 6. end to end -------------------------------------------------------------------------------------------------------
def _dataset(tmp_path):
    rs = np.random.RandomState(4)
    T, H, W = 12, 48, 40
    raw = rs.randint(50, 400, size=(T, H, W))
    masks = np.zeros((6, H, W), np.int8)
    for z in range(6):
        cy, cx = rs.randint(5, H - 5), rs.randint(5, W - 5)
        masks[z, cy - 2:cy + 3, cx - 2:cx + 3] = 1
        raw[:, cy - 2:cy + 3, cx - 2:cx + 3] += rs.randint(0, 3000, size=(T, 1, 1))      # a neuron: pixels that move together
    raw = raw.astype(np.int16)
    p = str(tmp_path / 'rec.npz')
    np.savez(p, series_raw=raw, series_mean=_mean16_ref(raw), masks_raw=masks, name=np.array('neurofinder.00.00'))
    return p, raw


def test_summarize_series_device_is_a_series_summary_func(tmp_path):
    from deep_calcium_amd import SeriesSummarizer, UNet2DSummary, summarize_series_device, unet_hip
    from deep_calcium_amd.series import KINDS
    from deep_calcium_amd.unet2ds import _summarize_series
    path, raw = _dataset(tmp_path)
    T, H, W = raw.shape
    host = _summarize_series(path)
    s = SeriesSummarizer((H, W), T, raw.dtype, chunk_frames=5)
    s.feed(raw)
    for kind in KINDS:
        for standardize in (False, True):
            got = summarize_series_device(path, kind=kind, standardize=standardize, chunk_frames=7)
            assert type(got) is type(host) and got.dtype == host.dtype == np.float32 and got.shape == host.shape == (H, W)
            assert np.array_equal(got, np.asarray(s.result(kind, standardize=standardize), np.float32)), (kind, standardize)
    # the default summary of the host path, from the raw frames: the standardised stored mean (the host function takes mean and
    # std in float32, good to ~1e-6 relative over 1920 pixels; the device in double)
    assert np.allclose(summarize_series_device(path, kind='mean16'), host, rtol=1e-5, atol=1e-5)
    assert summarize_series_device(path, kind='corr', standardize=False).max() > 0.5       # the planted neurons light up

    np.random.seed(3)
    model = UNet2DSummary(cpdir=str(tmp_path / 'cp'), net_builder_func=lambda shape: unet_hip(shape, nb_filters_base=4),
                          series_summary_func=functools.partial(summarize_series_device, kind='corr'))
    hist, _ = model.fit([path], shape_trn=(32, 32), shape_val=(64, 64), batch_size_trn=2, nb_steps_trn=2, nb_epochs=1)
    assert len(hist['loss']) == 1 and np.isfinite(hist['loss']).all()


# ---- 7. errors -----------------------------------------------------------------------------------------------------------
def test_errors_are_raised_before_any_launch(dclib):
    from deep_calcium_amd import SeriesSummarizer
    from deep_calcium_amd._lib import DcunetError
    s = SeriesSummarizer((5, 7), 4, np.int16, kinds=('mean', 'corr'))
    ok = np.zeros((2, 5, 7), np.int16)
    with pytest.raises(ValueError, match='uint16'):
        s.feed(ok.astype(np.uint16))
    with pytest.raises(ValueError, match=r'\(t, 5, 7\)'):
        s.feed(np.zeros((2, 7, 5), np.int16))
    with pytest.raises(ValueError, match='after 0 of 4'):
        s.result('mean')
    s.feed(ok)
    with pytest.raises(ValueError, match='declared to have 4'):
        s.feed(np.zeros((3, 5, 7), np.int16))
    assert s.fed == 2
    s.feed(ok)
    with pytest.raises(ValueError, match='not one of'):
        s.result('median')
    with pytest.raises(ValueError, match='not requested'):
        s.result('mean16')
    assert s.result('mean').shape == (5, 7)
    # the T limit of the int64 state, on the C ABI itself: refused with DC_EUNSUP, nothing launched
    st = _State(dclib, 5, 7, chain=False).run(ok, 2)
    with pytest.raises(DcunetError, match=r'\(-3\).*2147483647'):
        st.finalize(2 ** 31, corr=True)
    with pytest.raises(DcunetError, match=r'\(-3\)'):
        dclib.dc_series_accumulate(st.sum.data_ptr(), 0, 1, 0, 2 ** 31, None, None, st.sum.data_ptr(), st.sumsq.data_ptr(),
                                   st.vmax.data_ptr(), 5, 7, None)
    with pytest.raises(DcunetError, match=r'\(-1\)'):
        st.L.dc_series_finalize(st.sum.data_ptr(), st.sumsq.data_ptr(), None, None, None, st.sum.data_ptr(), 5, 7, 2, None)
