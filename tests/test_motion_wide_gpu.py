"""The wide (coarse-to-fine) shift search on the device (include/dcunet.h dc_motion_bin / dc_motion_ssd_around /
dc_motion_pick_around; MotionCorrector(coarse=), make_template(coarse=), estimate_shifts_device(coarse=)) against the integer
oracle of tests/_motion_wide_ref.py.  Every comparison is equality; every output buffer is pre-filled with garbage."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _motion_ref as ref             # noqa: E402
import _motion_sub_ref as sref        # noqa: E402
import _motion_wide_ref as wref       # noqa: E402

DTYPES = [np.int16, np.uint16]
I32_MAX = 2 ** 31 - 1


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32))).cuda()


def _rand(rs, shape, dtype):
    info = np.iinfo(dtype)
    return rs.randint(info.min, info.max + 1, size=shape).astype(dtype)


def _bin(L, frames, c, odd=0):
    """dc_motion_bin into a buffer of 0x5a5a with a guard behind it; odd: the frames start that many elements into their
    allocation (off 16-byte alignment: the value-by-value path)."""
    T, H, W = frames.shape
    Hc, Wc = H // c, W // c
    src = torch.zeros((frames.size + odd + 8,), dtype=torch.int16, device='cuda')
    src[odd:odd + frames.size] = _dev(frames).reshape(-1)
    buf = torch.full((T * Hc * Wc + 8,), 0x5a5a, dtype=torch.int16, device='cuda')
    L.dc_motion_bin(src.data_ptr() + 2 * odd, int(frames.dtype == np.uint16), T, H, W, c, buf.data_ptr(), _st())
    got = buf.cpu().numpy()
    assert (got[T * Hc * Wc:] == 0x5a5a).all()                    # nothing behind `out` is written
    return got[:T * Hc * Wc].reshape(T, Hc, Wc).view(frames.dtype)


def _around(L, frames, tmpl, S, D, rows, mult):
    """dc_motion_ssd_around into a table of garbage: every score must be written."""
    T, H, W = frames.shape
    nd = 2 * D + 1
    ws = torch.full((T * nd * nd + 4,), -7, dtype=torch.int64, device='cuda')
    df, dt, dr = _dev(frames), _dev(tmpl), _i32(rows)
    L.dc_motion_ssd_around(df.data_ptr(), int(frames.dtype == np.uint16), T, dt.data_ptr(), H, W, S, D, dr.data_ptr(), int(mult),
                           ws.data_ptr(), _st())
    got = ws.cpu().numpy()
    assert (got[T * nd * nd:] == -7).all()
    return got[:T * nd * nd].reshape(T, nd, nd)


def _ssd(L, frames, tmpl, S):
    T, H, W = frames.shape
    nd = 2 * S + 1
    sc = torch.full((T, nd, nd), -7, dtype=torch.int64, device='cuda')
    df, dt = _dev(frames), _dev(tmpl)
    L.dc_motion_ssd(df.data_ptr(), int(frames.dtype == np.uint16), T, dt.data_ptr(), H, W, S, sc.data_ptr(), _st())
    return sc.cpu().numpy()


def _pick_around(L, wscores, rows, mult, S, best=True, fine=True):
    T, nd = wscores.shape[:2]
    dw, dr = torch.from_numpy(np.array(wscores, np.int64)).cuda(), _i32(rows)
    sh = torch.full((T, 2), 12345, dtype=torch.int32, device='cuda')
    bs = torch.full((T,), -7, dtype=torch.int64, device='cuda')
    fn = torch.full((T, 2), 12345, dtype=torch.int32, device='cuda')
    L.dc_motion_pick_around(dw.data_ptr(), dr.data_ptr(), int(mult), T, S, (nd - 1) // 2, sh.data_ptr(), bs.data_ptr() if best else None,
                            fn.data_ptr() if fine else None, _st())
    return sh.cpu().numpy(), bs.cpu().numpy(), fn.cpu().numpy()


# ---- dc_motion_bin --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W,c,tc', [(8, 8, 2, 1), (9, 11, 2, 3), (37, 70, 4, 5), (64, 1040, 8, 2), (130, 67, 4, 33)])
@pytest.mark.parametrize('dtype', DTYPES)
def test_bin_equals_the_oracle(dclib, H, W, c, tc, dtype):
    rs = np.random.RandomState(H + W + c)
    frames = _rand(rs, (tc, H, W), dtype)
    assert (frames.astype(np.int64) > 32767).any() if dtype == np.uint16 else (frames < 0).any()
    want = wref.bin_frames(frames, c)
    assert want.shape == (tc, H // c, W // c)
    assert np.array_equal(_bin(dclib, frames, c), want)
    assert np.array_equal(_bin(dclib, frames, c, odd=1), want)            # the frames off 16-byte alignment
    # frames of all-maximum and all-minimum values keep them
    info = np.iinfo(dtype)
    for v in (info.min, info.max):
        const = np.full((tc, H, W), v, dtype)
        got = _bin(dclib, const, c)
        assert (got == v).all() and np.array_equal(got, wref.bin_frames(const, c))
    # small negative and positive sums: the floor and the half that rounds up
    near = rs.randint(-2, 3, size=(tc, H, W)).astype(np.int16).astype(dtype)
    assert np.array_equal(_bin(dclib, near, c), wref.bin_frames(near, c))


def test_every_factor_bins_the_same_frames(dclib):
    rs = np.random.RandomState(2)
    frames = _rand(rs, (3, 43, 88), np.int16)
    for c in (2, 4, 8):
        assert np.array_equal(_bin(dclib, frames, c), wref.bin_frames(frames, c))
    assert np.array_equal(_bin(dclib, np.array([[[-1, -1], [-1, -2]]], np.int16), 2), [[[-1]]])


# ---- dc_motion_ssd_around -------------------------------------------------------------------------------------------------------
def _centre_rows(rs, S, D, tc):
    """[(rows (n, 2), mult)]: the four corners +-(S - D), (0, 0), random rows, and rows at the int32 extremes with mult = 8."""
    M = S - D
    named = [(M, M), (M, -M), (-M, M), (-M, -M), (0, 0)]
    named += [tuple(int(v) for v in rs.randint(-S - 3, S + 4, size=2)) for _ in range(max(tc, 3))]
    out = []
    for a in range(0, len(named), tc):
        rows = (named[a:a + tc] + named[:tc])[:tc]
        out.append((np.array(rows, np.int64), 1))
    out.append((np.array([tuple(int(v) for v in rs.randint(-S // 2 - 1, S // 2 + 2, size=2)) for _ in range(tc)], np.int64), 2))
    extreme = [(I32_MAX, -I32_MAX), (-2 ** 31, I32_MAX), (I32_MAX, 0), (0, -2 ** 31), (-I32_MAX, -I32_MAX)]
    out.append((np.array((extreme * tc)[:tc], np.int64), 8))
    return out


@pytest.mark.parametrize('H,W,S,D,tc', [(40, 44, 8, 4, 3), (70, 150, 24, 2, 5), (60, 1100, 20, 4, 2), (300, 280, 128, 8, 2), (40, 40, 4, 0, 2)])
@pytest.mark.parametrize('dtype', DTYPES)
def test_window_scores_equal_the_oracle(dclib, H, W, S, D, tc, dtype):
    rs = np.random.RandomState(H + S + D)
    tmpl = _rand(rs, (H, W), dtype)
    frames = _rand(rs, (tc, H, W), dtype)
    full = _ssd(dclib, frames, tmpl, S) if S <= 16 else None
    if full is not None:
        assert np.array_equal(full, ref.scores(frames, tmpl, S))
    for rows, mult in _centre_rows(rs, S, D, tc):
        want = wref.window_scores(frames, tmpl, S, D, rows, mult)
        got = _around(dclib, frames, tmpl, S, D, rows, mult)
        assert np.array_equal(got, want), (rows.tolist(), mult)
        ctr = wref.centres(rows, mult, S, D)
        assert np.abs(ctr).max() <= S - D
        if full is not None:                             # the matching sub-block of the exhaustive table
            for k in range(tc):
                cy, cx = int(ctr[k, 0]), int(ctr[k, 1])
                assert np.array_equal(got[k], full[k, S + cy - D:S + cy + D + 1, S + cx - D:S + cx + D + 1])


@pytest.mark.parametrize('dtype', DTYPES)
def test_window_scores_at_the_extremes_of_the_range(dclib, dtype):
    """`hi` against `lo`: every difference is 65535, every score (H - 2S)(W - 2S) 65535^2."""
    H, W, S, D = 128, 256, 8, 2
    info = np.iinfo(dtype)
    rows = np.array([(3, -3), (-6, 6)])
    for a, b in ((info.min, info.max), (info.max, info.min)):
        tmpl, frames = np.full((H, W), a, dtype), np.full((2, H, W), b, dtype)
        got = _around(dclib, frames, tmpl, S, D, rows, 2)
        assert (got == (H - 2 * S) * (W - 2 * S) * 65535 ** 2).all()
        assert np.array_equal(got, wref.window_scores(frames, tmpl, S, D, rows, 2))


# ---- dc_motion_pick_around ------------------------------------------------------------------------------------------------------
def test_pick_orders_total_shifts(dclib):
    # centre (4, 0), D = 2, equal minima at the residuals (-2, 0) and (1, 0): the total shift (2, 0), not (5, 0)
    w = np.full((1, 5, 5), 100, np.int64)
    w[0, 0, 2] = w[0, 3, 2] = 7
    sh, bs, fn = _pick_around(dclib, w, [[1, 0]], 4, 6)
    assert sh.tolist() == [[2, 0]] and bs.tolist() == [7]
    assert fn.tolist() == [[32, 0]]                      # on the window's border along y: not refined
    # a constant table: the candidate of smallest total displacement, whatever the centre
    rows = np.array([[1, 0], [-3, 2], [0, 0], [5, -5], [I32_MAX, -2 ** 31]])
    const = np.full((5, 5, 5), 9, np.int64)
    sh, bs, fn = _pick_around(dclib, const, rows, 4, 20)
    want = wref.pick_around(const, rows, 4, 20)
    assert sh.tolist() == [[2, 0], [-10, 6], [0, 0], [16, -16], [16, -16]] and (bs == 9).all()
    assert np.array_equal(sh, want[0]) and np.array_equal(fn, 16 * sh) and np.array_equal(fn, want[2])


@pytest.mark.parametrize('D', [0, 1, 2, 4, 8])
def test_pick_and_fine_equal_the_oracle(dclib, D):
    rs = np.random.RandomState(D)
    T, nd, S = 33, 2 * D + 1, 16 * max(D, 1)
    w = (rs.randint(0, 2 ** 31, size=(T, nd, nd)).astype(np.int64) << 31) | rs.randint(0, 2 ** 31, size=(T, nd, nd))
    w[::3] >>= rs.randint(20, 60)
    w[1::4] = rs.randint(0, 3, size=w[1::4].shape)                       # heavily tied
    w[2, :, :] = 2 ** 62 - 1
    if D >= 1:
        w[5] = 10 ** 6
        w[5, 0, D] = 1                                   # a pick on the window's border along y, interior along x
        w[5, 0, D - 1], w[5, 0, D + 1] = 40, 20
        w[6] = 10 ** 6
        w[6, D, D] = 3                                   # an interior pick between unequal neighbours
        w[6, D - 1, D], w[6, D + 1, D], w[6, D, D - 1], w[6, D, D + 1] = 50, 3, 30, 90
    rows = rs.randint(-20, 21, size=(T, 2))
    rows[6], rows[7], rows[8] = (0, 0), (I32_MAX, -I32_MAX), (-2 ** 31, 0)           # table 6 ties (0, 0) with (1, 0): centred, (0, 0) wins
    mult = max(D, 1)
    want_sh, want_best, want_fine = wref.pick_around(w, rows, mult, S)
    sh, bs, fn = _pick_around(dclib, w, rows, mult, S)
    assert np.array_equal(sh, want_sh) and np.array_equal(bs, want_best) and np.array_equal(fn, want_fine)
    ctr = wref.centres(rows, mult, S, D)
    assert np.abs(want_sh - ctr).max() <= D and np.abs(want_fine - 16 * want_sh).max() <= 8
    if D >= 1:
        assert tuple(want_sh[5] - ctr[5]) == (-D, 0) and want_fine[5, 0] == 16 * want_sh[5, 0] and want_fine[5, 1] != 16 * want_sh[5, 1]
        assert tuple(want_sh[6] - ctr[6]) == (0, 0) and want_fine[6, 0] == 16 * want_sh[6, 0] + 8
    else:
        assert np.array_equal(want_fine, 16 * want_sh) and np.array_equal(want_sh, ctr)
    # best and fine are nullable: the other outputs do not change and the absent ones are not written
    sh2, bs2, fn2 = _pick_around(dclib, w, rows, mult, S, best=False, fine=False)
    assert np.array_equal(sh2, want_sh) and (bs2 == -7).all() and (fn2 == 12345).all()
    sh3, bs3, fn3 = _pick_around(dclib, w, rows, mult, S, best=False, fine=True)
    assert np.array_equal(sh3, want_sh) and (bs3 == -7).all() and np.array_equal(fn3, want_fine)


# ---- end to end -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('H,W,S,c', [(96, 112, 24, 4), (64, 80, 20, 2), (160, 176, 32, 8)])
@pytest.mark.parametrize('dtype', DTYPES)
def test_planted_offsets_are_recovered_and_corrected(H, W, S, c, dtype):
    from deep_calcium_amd import MotionCorrector
    tmpl, frames, offsets = wref.planted(H, W, S, c, dtype)
    want = wref.search(frames, tmpl, S, c)
    mc = MotionCorrector((H, W), len(frames), dtype, tmpl, max_shift=S, coarse=c)
    out = mc.feed(frames).cpu().numpy().view(dtype)
    shifts = mc.shifts()
    assert shifts.dtype == np.int32 and np.array_equal(shifts, want['shifts']) and np.array_equal(shifts, -offsets)
    assert np.abs(shifts).max() == S > 16
    assert np.array_equal(mc.coarse_shifts(), want['coarse']) and np.array_equal(mc.coarse_shifts_device().cpu().numpy(), want['coarse'])
    assert np.array_equal(mc.last_scores(), want['wscores']) and mc.last_scores().shape == (len(frames), 2 * c + 1, 2 * c + 1)
    assert np.array_equal(mc.last_coarse_scores(), want['cscores'])
    assert np.array_equal(out, ref.apply(frames, shifts, 0))
    (y0, y1), (x0, x1) = mc.valid()
    assert ((y0, y1), (x0, x1)) == ref.valid(shifts, (H, W)) == ((S, H - S), (S, W - S))
    assert (out[:, y0:y1, x0:x1] == tmpl[y0:y1, x0:x1]).all()
    # the same with sub-pixel refinement: the fine shifts are the oracle's, refined within the window table
    sub = MotionCorrector((H, W), len(frames), dtype, tmpl, max_shift=S, coarse=c, subpixel=True)
    out_s = sub.feed(frames).cpu().numpy().view(dtype)
    assert np.array_equal(sub.shifts(), shifts) and np.array_equal(sub.fine_shifts(), want['fine'])
    assert np.array_equal(out_s, sref.apply_sub(frames, want['fine'], 0))
    assert sub.valid() == sref.valid_fine(want['fine'], (H, W))


@pytest.mark.parametrize('dtype', DTYPES)
def test_coarse_2_agrees_with_the_exhaustive_search(dtype):
    from deep_calcium_amd import MotionCorrector
    H, W, S, c = 48, 52, 16, 2
    tmpl, frames, offsets = wref.planted(H, W, S, c, dtype)
    wide = MotionCorrector((H, W), len(frames), dtype, tmpl, max_shift=S, coarse=c)
    full = MotionCorrector((H, W), len(frames), dtype, tmpl, max_shift=S)
    out_w, out_f = wide.feed(frames), full.feed(frames)
    assert np.array_equal(wide.shifts(), full.shifts()) and np.array_equal(full.shifts(), -offsets)
    assert torch.equal(out_w, out_f)
    # the window table is the matching sub-block of the exhaustive table
    ws, fs = wide.last_scores(), full.last_scores()
    ctr = wref.centres(wide.coarse_shifts(), c, S, c)
    for k in range(len(frames)):
        cy, cx = int(ctr[k, 0]), int(ctr[k, 1])
        assert np.array_equal(ws[k], fs[k, S + cy - c:S + cy + c + 1, S + cx - c:S + cx + c + 1])


# ---- chunking, resident frames, dataset files -----------------------------------------------------------------------------------
H_, W_, S_, C_ = 64, 80, 20, 2


@pytest.fixture(scope='module')
def moving():
    """33 uint16 frames: the 32 planted ones and one more, every second one mixed 3 : 1 with the cut one column further (a quarter
    of a pixel, so that the refinement has work to do), and a little noise so that no score is 0; the ORACLE's tables and
    corrected frames: shared, never changed."""
    rs = np.random.RandomState(33)
    scene = rs.randint(0, 65536, size=(H_ + 2 * S_, W_ + 2 * S_)).astype(np.uint16)
    offsets = wref.planted(H_, W_, S_, C_, np.uint16)[2].tolist() + [(7, -19)]
    tmpl, frames = ref.cut(scene, H_, W_, S_, offsets)
    _, beside = ref.cut(scene, H_, W_, S_, [(a, b + 1 if b < S_ else b - 1) for a, b in offsets])
    frames[1::2] = ((3 * frames.astype(np.int64) + beside) // 4)[1::2].astype(np.uint16)
    frames = (frames.astype(np.int64) + rs.randint(-300, 301, size=frames.shape)).clip(0, 65535).astype(np.uint16)
    r = wref.search(frames, tmpl, S_, C_)
    assert np.array_equal(r['shifts'], -np.array(offsets)) and np.abs(r['shifts']).max() == S_ > 16
    assert (r['best'] > 0).all() and (r['fine'] != 16 * r['shifts']).any(axis=1).sum() >= 10
    r.update(tmpl=tmpl, frames=frames, out=ref.apply(frames, r['shifts'], 0), out_sub=sref.apply_sub(frames, r['fine'], 0))
    return r


def test_chunking_and_resident_frames_never_change_a_bit(moving):
    from deep_calcium_amd import MotionCorrector
    frames, tmpl = moving['frames'], moving['tmpl']
    T = len(frames)

    def run(parts, chunk_frames=None, device=False, subpixel=True):
        mc = MotionCorrector((H_, W_), T, np.uint16, tmpl, max_shift=S_, coarse=C_, chunk_frames=chunk_frames, subpixel=subpixel)
        outs, a = [], 0
        for n in parts:
            piece = frames[a:a + n]
            outs.append(mc.feed(_dev(piece) if device else piece))
            a += n
        assert np.array_equal(mc.shifts(), moving['shifts']) and np.array_equal(mc.coarse_shifts(), moving['coarse']), (parts, chunk_frames, device)
        if subpixel:
            assert np.array_equal(mc.fine_shifts(), moving['fine']), (parts, chunk_frames, device)
        return torch.cat(outs).cpu().numpy().view(np.uint16)
    for parts, cf in (((33,), None), ((1, 32), None), ((16, 17), None), ((33,), 5), ((33,), 7), ((16, 17), 5)):
        for device in (False, True):
            assert np.array_equal(run(parts, cf, device), moving['out_sub']), (parts, cf, device)
    assert np.array_equal(run((16, 17), 7, False, subpixel=False), moving['out'])
    # correct=False only estimates
    mc = MotionCorrector((H_, W_), T, np.uint16, tmpl, max_shift=S_, coarse=C_, chunk_frames=7)
    assert mc.feed(frames, correct=False) is None and np.array_equal(mc.shifts(), moving['shifts'])
    assert np.array_equal(mc.last_scores(), moving['wscores'][28:]) and np.array_equal(mc.last_coarse_scores(), moving['cscores'][28:])


def _wide_template(frames, S, c):
    """make_template(coarse=c, iterations=1) on the oracle."""
    t0 = ref.rounded_mean(frames)
    return ref.rounded_mean(ref.apply(frames, wref.search(frames, t0, S, c)['shifts'], 0))


def test_template_and_shifts_of_a_dataset_file(tmp_path, moving):
    from deep_calcium_amd import estimate_shifts_device, hdf5_min, make_template, summarize_series_device
    frames, tmpl = moving['frames'], moving['tmpl']
    T = len(frames)
    path, cpath = str(tmp_path / 'moving.hdf5'), str(tmp_path / 'corrected.hdf5')
    for p, data in ((path, frames), (cpath, moving['out'])):
        w = hdf5_min.Writer()
        w.create_dataset('series/raw', data=data)
        w.save(p)
    want_t = _wide_template(frames[:10], S_, C_)
    assert np.array_equal(make_template(frames[:10], max_shift=S_, iterations=1, coarse=C_), want_t)
    for cf in (None, 7):
        shifts, t = estimate_shifts_device(path, template=tmpl, max_shift=S_, coarse=C_, chunk_frames=cf)
        assert shifts.dtype == np.int32 and shifts.shape == (T, 2) and np.array_equal(shifts, moving['shifts'])
        fine, t = estimate_shifts_device(path, template=tmpl, max_shift=S_, coarse=C_, chunk_frames=cf, subpixel=True)
        assert np.array_equal(fine, moving['fine'])
    # without a template: built by the wide search from the first frames, then every frame registered to it
    shifts2, t2 = estimate_shifts_device(path, max_shift=S_, coarse=C_, template_frames=10)
    assert np.array_equal(t2, want_t) and np.array_equal(shifts2, wref.search(frames, want_t, S_, C_)['shifts'])
    # the consumers take shifts beyond 16 pixels as they are
    assert np.abs(shifts).max() > 16
    a = summarize_series_device(path, kind='max', standardize=False, shifts=shifts)
    assert np.array_equal(a, moving['out'].max(axis=0).astype(np.float32))
    for kind in ('mean', 'std'):
        a = summarize_series_device(path, kind=kind, shifts=shifts)
        b = summarize_series_device(cpath, kind=kind)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and not np.array_equal(a, summarize_series_device(path, kind=kind))
