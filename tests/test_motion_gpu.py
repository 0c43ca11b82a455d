"""Rigid motion correction on the device (include/dcunet.h dc_motion_ssd / dc_motion_pick / dc_motion_apply;
deep_calcium_amd/motion.py and the shifts= keyword of series.py / traces.py) against the numpy int64 oracle of tests/_motion_ref.py.
Every comparison is equality."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _motion_ref as ref      # noqa: E402

GARBAGE = -0x0123456789abcdef
DTYPES = [np.int16, np.uint16]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _rand(rs, shape, dtype):
    info = np.iinfo(dtype)
    return rs.randint(info.min, info.max + 1, size=shape).astype(dtype)


def _ssd(L, frames, tmpl, S):
    """dc_motion_ssd on caller-owned buffers filled with garbage: every score must be written."""
    T, H, W = frames.shape
    nd = 2 * S + 1
    sc = torch.full((T, nd, nd), GARBAGE, dtype=torch.int64, device='cuda')
    df, dt = _dev(frames), _dev(tmpl)
    L.dc_motion_ssd(df.data_ptr(), int(frames.dtype == np.uint16), T, dt.data_ptr(), H, W, S, sc.data_ptr(), _st())
    return sc


def _pick(L, sc, S, want_best=True):
    T = sc.shape[0]
    shifts = torch.full((T, 2), 12345, dtype=torch.int32, device='cuda')
    best = torch.full((T,), GARBAGE, dtype=torch.int64, device='cuda') if want_best else None
    L.dc_motion_pick(sc.data_ptr(), T, S, shifts.data_ptr(), best.data_ptr() if want_best else None, _st())
    return shifts, best


def _apply(L, frames, shifts, fill):
    T, H, W = frames.shape
    df = _dev(frames)
    ds = shifts if torch.is_tensor(shifts) else torch.from_numpy(np.asarray(shifts, np.int32)).cuda()
    out = torch.full((T, H, W), 0x5a5a, dtype=torch.int16, device='cuda')
    L.dc_motion_apply(df.data_ptr(), T, ds.data_ptr(), H, W, int(fill), out.data_ptr(), _st())
    return out.cpu().numpy().view(frames.dtype)


# (H, W, S, tc).  The tile of one workgroup is 512 interior columns (64 lanes x 8 pixels) x 32 interior rows (16 rows above S = 8);
# three kernel instantiations serve S <= 4, S <= 8 and S <= 16.  The issue's six shapes, then the edges of THIS tiling:
#   (11, 1040, 1, 2): the interior is 1038 columns -- three column tiles, the last one 14 pixels wide (one full lane, one of 6)
#   (37, 531, 9, 1):  S = 9 runs on the S <= 16 instantiation with windows shorter than its maximum; 513 interior columns leave a
#                     second tile ONE pixel wide, 19 interior rows are two row tiles of that instantiation
#   (21, 35, 5, 2):   S = 5 on the S <= 8 instantiation
#   (34, 528, 8, 2):  512 interior columns: every lane full, the path without the ragged-lane mask, all 64 lanes
SSD_SHAPES = [(9, 9, 4, 1), (19, 23, 3, 5), (37, 70, 8, 33), (70, 150, 2, 3), (40, 40, 0, 4), (40, 41, 16, 2),
              (11, 1040, 1, 2), (37, 531, 9, 1), (21, 35, 5, 2), (34, 528, 8, 2),
              (50, 560, 16, 1)]                          # S = 16: a full 512-column tile plus a 16-pixel one, two row tiles (16 + 2)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('H,W,S,tc', SSD_SHAPES)
def test_scores_equal_the_oracle(dclib, H, W, S, tc, dtype):
    rs = np.random.RandomState(H * 1000 + W + S)
    frames, tmpl = _rand(rs, (tc, H, W), dtype), _rand(rs, (H, W), dtype)
    got = _ssd(dclib, frames, tmpl, S).cpu().numpy()
    assert np.array_equal(got, ref.scores(frames, tmpl, S))


@pytest.mark.parametrize('dtype,lo,hi', [(np.uint16, 0, 65535), (np.int16, -32768, 32767)])
def test_scores_at_the_extremes_of_the_range(dclib, dtype, lo, hi):
    H, W, S, tc = 128, 256, 1, 2
    frames, tmpl = np.full((tc, H, W), hi, dtype), np.full((H, W), lo, dtype)
    got = _ssd(dclib, frames, tmpl, S).cpu().numpy()
    n = (H - 2 * S) * (W - 2 * S)
    assert n * 65535 ** 2 > 2 ** 46 and (got == n * 65535 ** 2).all(), got


# ---- planted shifts -----------------------------------------------------------------------------------------------------------
H0, W0, S0 = 37, 70, 8
OFFSETS = [(8, 8), (8, -8), (-8, 8), (-8, -8), (0, 0), (3, -7), (-5, 2), (8, -1), (-1, 0), (0, 6)]


@pytest.fixture(scope='module')
def planted():
    rs = np.random.RandomState(11)
    scene = _rand(rs, (H0 + 2 * S0, W0 + 2 * S0), np.uint16)
    tmpl, frames = ref.cut(scene, H0, W0, S0, OFFSETS)
    want = -np.asarray(OFFSETS, np.int32)
    return tmpl, frames, want


def _check_corrected(out, tmpl, want, fill):
    (y0, y1), (x0, x1) = ref.valid(want, tmpl.shape)
    assert (y0, y1, x0, x1) == (S0, H0 - S0, S0, W0 - S0)
    for t in range(len(want)):
        dy, dx = want[t]
        inside = np.zeros(tmpl.shape, bool)
        inside[max(0, -dy):min(H0, H0 - dy), max(0, -dx):min(W0, W0 - dx)] = True
        assert np.array_equal(out[t][inside], tmpl[inside]) and (out[t][~inside] == fill).all(), t
        assert np.array_equal(out[t, y0:y1, x0:x1], tmpl[y0:y1, x0:x1])


def test_planted_shifts_are_recovered_through_the_c_abi(dclib, planted):
    tmpl, frames, want = planted
    sc = _ssd(dclib, frames, tmpl, S0)
    shifts, best = _pick(dclib, sc, S0)
    assert np.array_equal(shifts.cpu().numpy(), want)
    assert (best.cpu().numpy() == 0).all()
    out = _apply(dclib, frames, shifts, 7)
    assert np.array_equal(out, ref.apply(frames, want, 7))
    _check_corrected(out, tmpl, want, 7)


def test_planted_shifts_are_recovered_by_motion_corrector(planted):
    from deep_calcium_amd import MotionCorrector
    tmpl, frames, want = planted
    mc = MotionCorrector((H0, W0), len(frames), np.uint16, tmpl, max_shift=S0, fill=7)
    out = mc.feed(frames)
    assert out.dtype == torch.int16 and out.is_cuda and tuple(out.shape) == frames.shape
    assert np.array_equal(mc.shifts(), want) and mc.shifts().dtype == np.int32
    assert np.array_equal(mc.shifts_device().cpu().numpy(), want)
    assert mc.valid() == ((S0, H0 - S0), (S0, W0 - S0))
    assert np.array_equal(mc.last_scores(), ref.scores(frames, tmpl, S0))
    _check_corrected(out.cpu().numpy().view(np.uint16), tmpl, want, 7)


# ---- the tie rule -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_ties_go_to_the_smallest_displacement(dclib, dtype):
    H, W, S = 20, 31, 4
    const = np.full((2, H, W), 1234, dtype)
    shifts, _ = _pick(dclib, _ssd(dclib, const, np.full((H, W), 77, dtype), S), S)
    assert (shifts.cpu().numpy() == 0).all()
    row = np.array([5, 900, 30000], dtype)[np.arange(W) % 3]               # period 3 along x: dx = -3, 0, 3 all score 0
    pattern = np.broadcast_to(row, (H, W)).copy()
    sc = _ssd(dclib, pattern[None], pattern, S)
    assert (sc.cpu().numpy()[0, :, [1, 4, 7]] == 0).all()
    shifts, best = _pick(dclib, sc, S)
    assert shifts.cpu().numpy().tolist() == [[0, 0]] and best.cpu().numpy().tolist() == [0]


def test_pick_on_handcrafted_scores(dclib):
    S, nd = 4, 9
    sc = np.full((5, nd, nd), 1000, np.int64)
    for dy, dx in ((0, 0), (-4, -4), (0, -1), (1, 0)):
        sc[0, dy + S, dx + S] = 10                       # equal minima that include (0, 0)
    sc[1, S, S - 3] = sc[1, S, S + 3] = 10               # (0, -3) and (0, 3) only
    sc[2, S - 1, S] = sc[2, S, S + 1] = 10               # (-1, 0) and (0, 1) only
    sc[3, S + 4, S + 4] = 9                              # a strict minimum far away beats a nearer, larger score
    sc[3, S, S] = 10
    sc[4] = np.arange(nd * nd).reshape(nd, nd)[::-1, ::-1] - 2 ** 40      # negative values order as integers: the last entry
    shifts, best = _pick(dclib, torch.from_numpy(sc).cuda(), S)
    assert shifts.cpu().numpy().tolist() == [[0, 0], [0, -3], [-1, 0], [4, 4], [4, 4]]
    assert np.array_equal(shifts.cpu().numpy(), ref.pick(sc))
    assert best.cpu().numpy().tolist() == [10, 10, 10, 9, -2 ** 40]
    shifts, _ = _pick(dclib, torch.from_numpy(sc).cuda(), S, want_best=False)       # best is nullable
    assert np.array_equal(shifts.cpu().numpy(), ref.pick(sc))
    for S in (0, 16):                                    # one candidate; more candidates than two rounds of the wave
        sc = np.random.RandomState(S).randint(0, 50, size=(7, 2 * S + 1, 2 * S + 1)).astype(np.int64)
        shifts, _ = _pick(dclib, torch.from_numpy(sc).cuda(), S)
        assert np.array_equal(shifts.cpu().numpy(), ref.pick(sc))


# ---- dc_motion_apply ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T,H,W', [(1, 9, 11), (33, 13, 15), (3, 16, 64)])
@pytest.mark.parametrize('dtype,fill', [(np.int16, 0), (np.int16, -2), (np.uint16, 48879)])
def test_apply_equals_the_oracle(dclib, T, H, W, dtype, fill):
    rs = np.random.RandomState(T + H)
    frames = _rand(rs, (T, H, W), dtype)
    special = [(0, 0), (1, -1), (-3, 5), (2, 3), (0, 1), (0, -7), (H, 0), (-H, 0), (0, W), (0, -W), (H - 1, W - 1), (1 - H, 1 - W),
               (H - 1, 0), (0, 1 - W), (2 ** 31 - 1, 0), (0, -2 ** 31), (-2 ** 31, 2 ** 31 - 1), (5, 8), (-5, -8), (0, 16)]
    for base in range(0, len(special), T):               # every special shift meets some frame; T = 33 adds random ones
        shifts = np.array([special[(base + t) % len(special)] if t < len(special) else (rs.randint(-H, H + 1), rs.randint(-W, W + 1))
                           for t in range(T)], np.int64)
        want = ref.apply(frames, shifts, fill)
        assert np.array_equal(_apply(dclib, frames, shifts.astype(np.int32), fill), want)
    all_fill = ref.apply(frames[:1], [(H, 0)], fill)
    assert (all_fill == np.array(fill).astype(dtype)).all()


# ---- chunking -----------------------------------------------------------------------------------------------------------------
def test_chunking_never_changes_a_bit():
    from deep_calcium_amd import MotionCorrector
    rs = np.random.RandomState(5)
    H, W, S, T = 37, 70, 8, 33
    scene = _rand(rs, (H + 2 * S, W + 2 * S), np.uint16)
    offs = [(rs.randint(-S, S + 1), rs.randint(-S, S + 1)) for _ in range(T)]
    tmpl, frames = ref.cut(scene, H, W, S, offs)
    frames = frames + rs.randint(0, 3, size=frames.shape).astype(np.uint16)       # noise: non-zero scores
    want_s = ref.pick(ref.scores(frames, tmpl, S))
    want = ref.apply(frames, want_s, 0)

    def run(parts, chunk_frames=None, device=False):
        mc = MotionCorrector((H, W), T, np.uint16, tmpl, max_shift=S, chunk_frames=chunk_frames)
        outs, a = [], 0
        for n in parts:
            piece = frames[a:a + n]
            outs.append(mc.feed(_dev(piece) if device else piece))
            a += n
        return mc.shifts(), torch.cat(outs).cpu().numpy().view(np.uint16)
    for parts, cf, device in (((33,), None, False), ((1, 32), None, False), ((16, 17), None, False), ((33,), 5, False),
                              ((33,), None, True), ((16, 17), 7, True)):
        s, out = run(parts, cf, device)
        assert np.array_equal(s, want_s) and np.array_equal(out, want), (parts, cf, device)


# ---- downstream ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def moving():
    rs = np.random.RandomState(9)
    H, W, S, T = 24, 36, 4, 21
    scene = (rs.randint(-3000, 3000, size=(H + 2 * S, W + 2 * S))).astype(np.int16)
    offs = [(rs.randint(-3, 4), rs.randint(-3, 4)) for _ in range(T)]
    tmpl, frames = ref.cut(scene, H, W, S, offs)
    frames = (frames + rs.randint(-40, 40, size=frames.shape)).astype(np.int16)
    shifts = ref.pick(ref.scores(frames, tmpl, S))
    assert np.array_equal(shifts, -np.asarray(offs))
    return frames, shifts, ref.apply(frames, shifts, 0)


def _summaries(frames, kinds, feed=None, **kw):
    from deep_calcium_amd import SeriesSummarizer
    summ = SeriesSummarizer(frames.shape[1:], len(frames), frames.dtype, kinds=kinds, **kw)
    for a in range(0, len(frames), 8):
        summ.feed(feed(frames[a:a + 8]) if feed else frames[a:a + 8])
    return [summ.result(k) for k in kinds]


def test_summarizer_applies_shifts_on_the_way_in(moving):
    frames, shifts, corrected = moving
    kinds = ('mean', 'std', 'corr')
    want = _summaries(corrected, kinds)
    for s in (shifts, shifts.astype(np.int64), torch.from_numpy(shifts).cuda()):
        for cf in (None, 5):
            got = _summaries(frames, kinds, shifts=s, chunk_frames=cf)
            for g, w in zip(got, want):
                assert g.dtype == np.float32 and np.array_equal(g.view(np.uint32), w.view(np.uint32))
    # shifts=None: what it was -- the summaries of the frames as they are
    plain = _summaries(frames, kinds + ('max',))
    assert np.array_equal(plain[3], frames.max(0).astype(np.float32))
    zero = _summaries(frames, kinds + ('max',), shifts=np.zeros_like(shifts))
    for g, w in zip(zero, plain):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
    assert not np.array_equal(plain[0], want[0])
    # a device tensor goes straight in
    fed = _summaries(frames, kinds, feed=_dev)
    for g, w in zip(fed, plain):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))
    fed = _summaries(frames, kinds, feed=_dev, shifts=shifts, chunk_frames=3)
    for g, w in zip(fed, want):
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32))


def test_trace_extractor_applies_shifts_on_the_way_in(moving):
    from deep_calcium_amd import RoiTraceExtractor
    frames, shifts, corrected = moving
    T, H, W = frames.shape
    rois = [np.argwhere(np.ones((5, 6), bool)) + (3, 4), np.argwhere(np.ones((H, W), bool)), np.array([[0, 0], [H - 1, W - 1]])]

    def sums(x, feed=None, **kw):
        ext = RoiTraceExtractor((H, W), T, np.int16, rois, **kw)
        for a in range(0, T, 8):
            ext.feed(feed(x[a:a + 8]) if feed else x[a:a + 8])
        return ext.result('sum'), ext.result('zscore')

    def numpy_sums(x):
        return np.stack([x.astype(np.int64)[:, r[:, 0], r[:, 1]].sum(1) for r in rois])
    want = sums(corrected)
    assert np.array_equal(want[0], numpy_sums(corrected))
    for got in (sums(frames, shifts=shifts), sums(frames, shifts=torch.from_numpy(shifts).cuda(), chunk_frames=5),
                sums(frames, feed=_dev, shifts=shifts, chunk_frames=3)):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    plain = sums(frames)
    assert np.array_equal(plain[0], numpy_sums(frames)) and not np.array_equal(plain[0], want[0])


# ---- make_template and estimate_shifts_device ---------------------------------------------------------------------------------
def test_make_template_and_estimate_shifts_on_a_dataset_file(tmp_path):
    from deep_calcium_amd import (estimate_shifts_device, extract_traces_device, hdf5_min, make_template,
                                  summarize_series_device)
    rs = np.random.RandomState(21)
    T, H, W, S = 24, 40, 48, 4
    scene = rs.randint(0, 4000, size=(H + 2 * S, W + 2 * S)).astype(np.int16)
    offs = [(rs.randint(-2, 3), rs.randint(-2, 3)) for _ in range(T)]
    _, frames = ref.cut(scene, H, W, S, offs)
    frames = (frames + rs.randint(-20, 20, size=frames.shape)).astype(np.int16)
    path = str(tmp_path / 'moving.hdf5')
    w = hdf5_min.Writer()
    w.create_dataset('series/raw', data=frames)
    w.save(path)
    for dtype in DTYPES:
        x = frames.astype(dtype)
        assert np.array_equal(make_template(x, max_shift=S, iterations=0), ref.rounded_mean(x))
        got = make_template(x, max_shift=S, iterations=1)
        assert got.dtype == dtype and np.array_equal(got, ref.make_template(x, S, 1))
    want_t = ref.make_template(frames, S, 1)
    want_s = ref.pick(ref.scores(frames, want_t, S))
    for cf in (None, 7):
        shifts, tmpl = estimate_shifts_device(path, max_shift=S, chunk_frames=cf)
        assert np.array_equal(tmpl, want_t) and np.array_equal(shifts, want_s) and shifts.dtype == np.int32
    assert len(set(map(tuple, want_s.tolist()))) > 4                       # the frames do move
    # a template built from the first frames only, and a template that is given
    want_t10 = ref.make_template(frames[:10], S, 1)
    shifts, tmpl = estimate_shifts_device(path, max_shift=S, template_frames=10)
    assert np.array_equal(tmpl, want_t10) and np.array_equal(shifts, ref.pick(ref.scores(frames, want_t10, S)))
    shifts, tmpl = estimate_shifts_device(path, template=frames[3], max_shift=S)
    assert tmpl is frames[3] or np.array_equal(tmpl, frames[3])
    assert np.array_equal(shifts, ref.pick(ref.scores(frames, frames[3], S)))
    # and the one-call functions take them
    corrected = ref.apply(frames, want_s, 0)
    cpath = str(tmp_path / 'corrected.hdf5')
    w = hdf5_min.Writer()
    w.create_dataset('series/raw', data=corrected)
    w.save(cpath)
    a = summarize_series_device(path, kind='std', shifts=want_s)
    b = summarize_series_device(cpath, kind='std')
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    mask = np.zeros((H, W), np.uint8)
    mask[5:12, 7:15] = 1
    mask[20:30, 30:41] = 1
    a = extract_traces_device(path, mask, kind='sum', shifts=want_s)
    b = extract_traces_device(cpath, mask, kind='sum')
    assert np.array_equal(a, b) and not np.array_equal(a, extract_traces_device(path, mask, kind='sum'))
