"""Sub-pixel motion correction on the device (include/dcunet.h dc_motion_refine / dc_motion_block_refine / dc_motion_apply_sub /
dc_motion_warp_sub; MotionCorrector(subpixel=True), estimate_shifts_device(subpixel=True) and fine_shifts= in series.py /
traces.py) against the integer oracle of tests/_motion_sub_ref.py.  Every comparison is equality; every output buffer is
pre-filled with garbage."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _motion_block_ref as bref      # noqa: E402
import _motion_ref as ref             # noqa: E402
import _motion_sub_ref as sref        # noqa: E402

TOP = 2 ** 62 - 1                     # the largest score
DTYPE_FILL = [(np.int16, 0), (np.int16, -2), (np.uint16, 48879)]


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.int32))).cuda()


def _rand(rs, shape, dtype):
    info = np.iinfo(dtype)
    return rs.randint(info.min, info.max + 1, size=shape).astype(dtype)


def _refine(L, scores, shifts):
    """dc_motion_refine into a buffer of garbage: every row must be written."""
    T, nd = scores.shape[:2]
    fine = torch.full((T, 2), 12345, dtype=torch.int32, device='cuda')
    ds, dp = torch.from_numpy(np.array(scores, np.int64)).cuda(), _i32(shifts)
    L.dc_motion_refine(ds.data_ptr(), dp.data_ptr(), T, (nd - 1) // 2, fine.data_ptr(), _st())
    return fine.cpu().numpy()


def _block_refine(L, bscores, rigid, bshifts, S):
    T, By, Bx, nd = bscores.shape[:4]
    fine = torch.full((T, By, Bx, 2), 12345, dtype=torch.int32, device='cuda')
    ds, dr, db = torch.from_numpy(np.array(bscores, np.int64)).cuda(), _i32(rigid), _i32(bshifts)
    L.dc_motion_block_refine(ds.data_ptr(), dr.data_ptr(), db.data_ptr(), T, By, Bx, S, (nd - 1) // 2, fine.data_ptr(), _st())
    return fine.cpu().numpy()


def _into(frames, odd, launch):
    """`launch(out pointer)` into a buffer of 0x5a5a; odd: `out` starts that many elements into its allocation (the narrow path)."""
    T, H, W = frames.shape
    buf = torch.full((T * H * W + odd + 8,), 0x5a5a, dtype=torch.int16, device='cuda')
    launch(buf.data_ptr() + 2 * odd)
    got = buf.cpu().numpy()
    assert (got[:odd] == 0x5a5a).all() and (got[odd + T * H * W:] == 0x5a5a).all()           # nothing outside `out` is written
    return got[odd:odd + T * H * W].reshape(T, H, W).view(frames.dtype)


def _apply_sub(L, frames, fine, fill, odd=0):
    T, H, W = frames.shape
    df, ds, uns = _dev(frames), _i32(fine), int(frames.dtype == np.uint16)
    return _into(frames, odd, lambda out: L.dc_motion_apply_sub(df.data_ptr(), uns, T, ds.data_ptr(), H, W, int(fill), out, _st()))


def _warp_sub(L, frames, fbs, fill, odd=0):
    T, H, W = frames.shape
    By, Bx = np.asarray(fbs).shape[1:3]
    df, ds, uns = _dev(frames), _i32(fbs), int(frames.dtype == np.uint16)
    return _into(frames, odd, lambda out: L.dc_motion_warp_sub(df.data_ptr(), uns, T, ds.data_ptr(), By, Bx, H, W, int(fill), out, _st()))


def _apply(L, frames, shifts, fill):
    T, H, W = frames.shape
    df, ds = _dev(frames), _i32(shifts)
    return _into(frames, 0, lambda out: L.dc_motion_apply(df.data_ptr(), T, ds.data_ptr(), H, W, int(fill), out, _st()))


def _warp(L, frames, bs, fill):
    T, H, W = frames.shape
    By, Bx = np.asarray(bs).shape[1:3]
    df, ds = _dev(frames), _i32(bs)
    return _into(frames, 0, lambda out: L.dc_motion_warp(df.data_ptr(), T, ds.data_ptr(), By, Bx, H, W, int(fill), out, _st()))


# ---- dc_motion_refine -----------------------------------------------------------------------------------------------------------
def _table(S, pick, s0, ym, yp, xm, xp, rest):
    """A (2S+1)^2 table of `rest` with s0 at `pick` and the four neighbours given (None: not set, or outside the table)."""
    nd = 2 * S + 1
    t = np.full((nd, nd), rest, np.int64)
    i, j = pick[0] + S, pick[1] + S
    t[i, j] = s0
    for (a, b), v in (((i - 1, j), ym), ((i + 1, j), yp), ((i, j - 1), xm), ((i, j + 1), xp)):
        if v is not None and 0 <= a < nd and 0 <= b < nd:
            t[a, b] = v
    return t


def handmade(S):
    """[(table, the q expected at its pick or None)]: the named cases of the refinement.  With S = 0 every pick lies on the border."""
    if S == 0:
        return [(np.array([[v]], np.int64), (0, 0)) for v in (0, 7, TOP)]
    out = [(_table(S, (0, 0), 5, 100, 100, 9, 9, 10 ** 6), (0, 0)),                 # symmetric neighbourhoods
           (np.full((2 * S + 1, 2 * S + 1), 77, np.int64), (0, 0)),                 # flat: D = 0
           (_table(S, (0, 0), 3, 3, 50, 50, 3, 10 ** 6), (-8, 8)),                  # sm == s0 < sp: exactly -8; its mirror: +8
           # the tie at half a sixteenth goes to the pick.  N and D have the same parity (D - N = 2 (sp - s0)), so
           # N = 1, D = 16 cannot come from three scores: N = +-2, D = 32 is the same ratio; N = +-6, D = 32 is the tie at 1.5
           (_table(S, (0, 0), 0, 17, 15, 15, 17, 10 ** 6), (0, 0)),
           (_table(S, (0, 0), 0, 19, 13, 13, 19, 10 ** 6), (1, -1)),
           (_table(S, (0, 0), 1, 11, 8, 8, 11, 10 ** 6), (1, -1)),                  # N = +-3, D = 17: just beyond a half
           (_table(S, (0, 0), 0, TOP, TOP, TOP, 0, TOP), (0, 8)),                   # 0 and 2^62 - 1 side by side
           (_table(S, (0, 0), 0, TOP, TOP - 1, TOP // 2, TOP, TOP), (0, None)),
           (_table(S, (0, 0), 0, 16, 0, 4, 12, 10 ** 6), (8, -4))]                  # half and quarter of a pixel
    for pick in ((-S, 0), (S, 0), (0, -S), (0, S), (S, -S), (-S, -S), (S, S)):      # a pick on each border and in the corners
        t = _table(S, pick, 1, 40, 20, 30, 90, 10 ** 6)
        out.append((t, None))
    return out


@pytest.mark.parametrize('S', [0, 1, 3, 16])
def test_refine_on_handmade_tables(dclib, S):
    rs = np.random.RandomState(S)
    cases = handmade(S)
    tables = np.stack([t for t, _ in cases])
    picks = ref.pick(tables)
    want = sref.refine(tables, picks)
    for k, (t, q) in enumerate(cases):
        for c, v in enumerate(q or ()):
            assert v is None or (picks[k][c] == 0 and want[k][c] == v), (k, c)
        for c in (0, 1):                                 # a pick on the border of an axis is not refined on it
            if abs(picks[k][c]) == S:
                assert want[k][c] == 16 * picks[k][c]
        assert np.array_equal(_refine(dclib, t[None], picks[k:k + 1]), want[k:k + 1]), k           # tc = 1
    # tc = 33: the cases, then random tables whose scores span all 62 bits
    nd = 2 * S + 1
    more = (rs.randint(0, 2 ** 31, size=(33, nd, nd)).astype(np.int64) << 31) | rs.randint(0, 2 ** 31, size=(33, nd, nd))
    more[::3] >>= rs.randint(0, 60)
    tables = np.concatenate([tables, more])[:33]
    picks = ref.pick(tables)
    want = sref.refine(tables, picks)
    assert np.abs(want - 16 * picks).max() <= 8
    assert np.array_equal(_refine(dclib, tables, picks), want)
    # the mirror image of every table gives the mirrored fine shift
    assert np.array_equal(_refine(dclib, tables[:, ::-1, ::-1], -picks), -want)
    # rows no pick writes: outside the table nothing is read and q = 0
    far = picks.copy()
    far[:, 0] = S + 1 + np.abs(picks[:, 0])
    far[1::2] = (-40, 1000)
    assert np.array_equal(_refine(dclib, tables, far), 16 * far)


@pytest.mark.parametrize('tc,By,Bx,D', [(3, 2, 3, 2), (2, 1, 1, 0), (2, 4, 1, 8)])
def test_block_refine_equals_the_oracle(dclib, tc, By, Bx, D):
    rs = np.random.RandomState(D)
    S, nd = 3, 2 * D + 1
    bsc = (rs.randint(0, 2 ** 31, size=(tc, By, Bx, nd, nd)).astype(np.int64) << rs.randint(0, 32)) + rs.randint(0, 1000, size=(tc, By, Bx, nd, nd))
    if D >= 2:                                           # one block with an interior minimum between two unequal neighbours
        bsc[0, 0, 0, D, D] = 0
    rigid = np.array([(1000, -1000), (-2, 3), (-2 ** 31, 2 ** 31 - 1)], np.int64)[:tc]      # beyond +-S: clamped
    bs, _ = bref.block_pick(bsc, rigid, S)
    bs = bs.astype(np.int64)
    bs[-1, -1, -1] += (2 * D + 1, 0)                     # an inconsistent row: the residual lies outside [-D, D]
    want = sref.block_refine(bsc, rigid, bs, S)
    assert tuple(want[-1, -1, -1]) == tuple(16 * bs[-1, -1, -1])
    assert np.abs(want - 16 * bs).max() <= 8 and (D == 0 or (want != 16 * bs).any())
    assert np.array_equal(_block_refine(dclib, bsc, rigid, bs, S), want)
    if D == 0:
        assert np.array_equal(want, 16 * bs)


# ---- dc_motion_apply_sub --------------------------------------------------------------------------------------------------------
def _fine_specials(H, W):
    """The fine shifts every shape is tested at, for an H x W frame."""
    one = [0, 1, -1, 15, -15, 16, -16, 17, -17]
    out = [(a, b) for a, b in zip(one, one[::-1])] + [(a, 0) for a in one[1:]] + [(0, b) for b in one[1:]]
    out += [(-1, 15), (15, -1), (8, 8), (-40, 23), (5, 40)]
    out += [(32, -48), (-16, 16), (16 * (H - 1), 0), (0, 16 * (1 - W))]                     # multiples of 16
    # the i = 1 tap of output row H - 4 exactly on row H - 1 (row H - 3 fills); with fy = 0 one row further it does not fill
    out += [(37, 0), (48, 0), (0, 37), (0, 48), (37, 37), (16 * (H - 2) + 1, 16 * (W - 2) + 15), (16 * (H - 1), 16 * (W - 1))]
    # beyond the frame: all fill
    out += [(16 * H, 0), (-16 * H, 0), (0, 16 * W), (0, -16 * W - 1), (16 * (H - 1) + 1, 0), (0, 16 * (W - 1) + 1), (-16 * H + 15, 0),
            (2 ** 31 - 1, 0), (0, -2 ** 31), (-2 ** 31, 2 ** 31 - 1), (2 ** 31 - 1, -2 ** 31)]
    return out


def test_the_edge_rows_of_the_oracle():
    """What the edge shifts of _fine_specials are there for, on the oracle: no pixel of the frame equals the fill."""
    H, W = 9, 11
    f = np.arange(1, H * W + 1, dtype=np.int16).reshape(1, H, W)
    filled = lambda s: sref.apply_sub(f, [s], -7)[0] == -7          # noqa: E731
    assert not filled((37, 0))[H - 4].any() and filled((37, 0))[H - 3].all() and not filled((48, 0))[H - 4].any()
    assert not filled((0, 37))[:, W - 4].any() and filled((0, 37))[:, W - 3].all() and not filled((0, 48))[:, W - 4].any()
    assert not filled((16 * (H - 1), 16 * (W - 1)))[0, 0] and filled((16 * (H - 1), 16 * (W - 1))).sum() == H * W - 1
    for s in ((16 * H, 0), (0, -16 * W - 1), (16 * (H - 1) + 1, 0), (0, 16 * (W - 1) + 1), (-16 * H + 15, 0), (2 ** 31 - 1, -2 ** 31)):
        assert filled(s).all(), s
    assert not filled((-16 * H + 16, 0))[H - 1].any()


@pytest.mark.parametrize('T,H,W', [(1, 9, 11), (33, 13, 15), (3, 16, 64), (2, 40, 1100)])
@pytest.mark.parametrize('dtype,fill', DTYPE_FILL)
def test_apply_sub_equals_the_oracle(dclib, T, H, W, dtype, fill):
    rs = np.random.RandomState(T + H)
    frames = _rand(rs, (T, H, W), dtype)
    assert (frames.astype(np.int64) > 32767).any() if dtype == np.uint16 else (frames < 0).any()
    special = _fine_specials(H, W)
    for base in range(0, len(special), T):               # every special shift meets every shape
        fine = np.array([special[(base + k) % len(special)] for k in range(T)], np.int64)
        want = sref.apply_sub(frames, fine, fill)
        assert np.array_equal(_apply_sub(dclib, frames, fine, fill), want), base
        assert np.array_equal(_apply_sub(dclib, frames, fine, fill, odd=3), want), base           # out off 16-byte alignment
        whole = (fine % 16 == 0).all(axis=1)
        if whole.any():                                  # multiples of 16: dc_motion_apply bit for bit
            moved = _apply(dclib, frames, fine // 16 * whole[:, None], fill)
            assert np.array_equal(want[whole], moved[whole])


@pytest.mark.parametrize('dtype,value', [(np.uint16, 65535), (np.int16, -32768), (np.int16, 32767), (np.uint16, 0)])
def test_a_constant_frame_stays_constant_at_fractional_shifts(dclib, dtype, value):
    T, H, W = 5, 13, 40
    frames = np.full((T, H, W), value, dtype)
    fine = np.array([(1, 1), (15, -15), (-8, 8), (-17, 23), (7, 0)])
    fill = 1234
    got = _apply_sub(dclib, frames, fine, fill)
    assert np.array_equal(got, sref.apply_sub(frames, fine, fill))
    assert set(np.unique(got).tolist()) == {value, fill}
    (y0, y1), (x0, x1) = sref.valid_fine(fine, (H, W))
    assert (got[:, y0:y1, x0:x1] == value).all()


# ---- dc_motion_warp_sub ---------------------------------------------------------------------------------------------------------
def _fine_blocks(rs, T, By, Bx, H, W, base):
    special = _fine_specials(H, W)
    n = T * By * Bx
    flat = [special[(base + k) % len(special)] if k < len(special) else
            (special[rs.randint(len(special))] if rs.randint(4) == 0 else (rs.randint(-60, 61), rs.randint(-60, 61))) for k in range(n)]
    return np.array(flat, np.int64).reshape(T, By, Bx, 2)


@pytest.mark.parametrize('T,H,W', [(1, 9, 11), (33, 13, 15), (3, 16, 64)])
@pytest.mark.parametrize('By,Bx', [(1, 1), (2, 3), (4, 1)])
@pytest.mark.parametrize('dtype,fill', DTYPE_FILL)
def test_warp_sub_equals_the_oracle(dclib, T, H, W, By, Bx, dtype, fill):
    rs = np.random.RandomState(T + H + By)
    frames = _rand(rs, (T, H, W), dtype)
    n = T * By * Bx
    for base in range(0, len(_fine_specials(H, W)), n):
        fbs = _fine_blocks(rs, T, By, Bx, H, W, base)
        want = sref.warp_sub(frames, fbs, fill)
        assert np.array_equal(_warp_sub(dclib, frames, fbs, fill), want), base
        if base == 0:
            assert np.array_equal(_warp_sub(dclib, frames, fbs, fill, odd=3), want)        # out off 16-byte alignment
    # a smooth field, as the refinement gives it: block shifts a few sixteenths apart around the frame's own
    fbs = rs.randint(-12, 13, size=(T, By, Bx, 2)) + rs.randint(-50, 51, size=(T, 1, 1, 2))
    assert np.array_equal(_warp_sub(dclib, frames, fbs, fill), sref.warp_sub(frames, fbs, fill))


def test_warp_sub_of_a_smooth_field_over_several_tiles(dclib):
    """Tiles of 16 rows x 1024 columns: (2, 35, 520) in 32 x 32 blocks and (2, 40, 1100) in 3 x 4."""
    for T, H, W, By, Bx in ((2, 35, 520, 32, 32), (2, 40, 1100, 3, 4)):
        rs = np.random.RandomState(W)
        frames = _rand(rs, (T, H, W), np.int16)
        fbs = rs.randint(-20, 21, size=(T, By, Bx, 2)) + rs.randint(-90, 91, size=(T, 1, 1, 2))
        want = sref.warp_sub(frames, fbs, -9)
        assert np.array_equal(_warp_sub(dclib, frames, fbs, -9), want)
        assert np.array_equal(_warp_sub(dclib, frames, fbs, -9, odd=1), want)


@pytest.mark.parametrize('By,Bx', [(1, 1), (2, 3), (4, 1)])
def test_equal_fine_block_shifts_are_dc_motion_apply_sub(dclib, By, Bx):
    rs = np.random.RandomState(By)
    for T, H, W in ((1, 9, 11), (33, 13, 15), (3, 16, 64)):
        frames = _rand(rs, (T, H, W), np.int16)
        special = _fine_specials(H, W)
        fine = np.array([special[(5 * t + By) % len(special)] for t in range(T)], np.int64)
        fbs = np.broadcast_to(fine[:, None, None, :], (T, By, Bx, 2))
        got = _warp_sub(dclib, frames, fbs, -2)
        assert np.array_equal(got, _apply_sub(dclib, frames, fine, -2)) and np.array_equal(got, sref.apply_sub(frames, fine, -2))


@pytest.mark.parametrize('By,Bx', [(1, 1), (2, 3), (4, 1)])
def test_whole_pixel_fine_block_shifts_against_dc_motion_warp(dclib, By, Bx):
    """Fine block shifts that are multiples of 16.  Where a frame's block shifts are equal the output is dc_motion_warp's bit for
    bit.  Where they differ, the two agree at every pixel at which the fine field is itself a multiple of 16, and only there
    by definition: between two block centres one pixel apart the fine field passes through every sixteenth (that is what it is
    for) while the whole-pixel field of dc_motion_warp jumps -- so 'all multiples of 16 make it dc_motion_warp' cannot
    hold together with the field's definition, and the identity is asserted in the form that does."""
    rs = np.random.RandomState(By + 7)
    for T, H, W in ((1, 9, 11), (33, 13, 15), (3, 16, 64), (2, 35, 520)):
        frames = _rand(rs, (T, H, W), np.uint16)
        shifts = rs.randint(-3, 4, size=(T, 1, 1, 2))
        bs = np.broadcast_to(shifts, (T, By, Bx, 2))
        assert np.array_equal(_warp_sub(dclib, frames, 16 * bs, 9), _warp(dclib, frames, bs, 9))
        bs = shifts + rs.randint(-2, 3, size=(T, By, Bx, 2))
        got, moved = _warp_sub(dclib, frames, 16 * bs, 9), _warp(dclib, frames, bs, 9)
        whole = np.stack([(sref.fine_field(16 * bs[t], H, W) % 16 == 0).all(-1) for t in range(T)])
        assert whole.any() and np.array_equal(got[whole], moved[whole])
        assert np.array_equal(got, sref.warp_sub(frames, 16 * bs, 9))


# ---- planted sub-pixel motion ---------------------------------------------------------------------------------------------------
def scene(H, W, oy, ox, base=8000.0):
    """A smooth scene sampled analytically at (y + oy, x + ox), rounded to uint16, no noise."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    y, x = y + oy, x + ox
    v = base + 3000 * np.sin(y / 5.3 + 0.3) * np.cos(x / 4.1) + 2000 * np.sin((y + x) / 7.7) + 1500 * np.cos(y / 3.1 - x / 6.3)
    return np.rint(v).astype(np.uint16)


OFFSETS = [(0.5, 0.5), (-0.5, 0.25), (1.5, -1.5), (0.25, 0.75), (-2.4375, 1.0625), (0.0625, -0.0625), (0, 0.5)]


def test_planted_subpixel_motion_is_recovered_and_corrected():
    """Conditions on the inputs, re-checked on the oracle alone before any device saw them: the worst error of the fine shifts is
    2 sixteenths and the squared difference to the template falls by a factor of 11 to 55."""
    from deep_calcium_amd import MotionCorrector
    H, W, S, m = 40, 48, 3, 4
    tmpl = scene(H, W, 0, 0)
    frames = np.stack([scene(H, W, oy, ox) for oy, ox in OFFSETS])
    sc = ref.scores(frames, tmpl, S)
    pk = ref.pick(sc)
    want = sref.refine(sc, pk)
    assert (np.abs(pk) < S).all()                        # no pick on the table's border, where q = 0 by definition
    sub = MotionCorrector((H, W), len(frames), np.uint16, tmpl, max_shift=S, subpixel=True)
    out_s = sub.feed(frames).cpu().numpy().view(np.uint16)
    whole = MotionCorrector((H, W), len(frames), np.uint16, tmpl, max_shift=S)
    out_w = whole.feed(frames).cpu().numpy().view(np.uint16)
    fine = sub.fine_shifts()
    assert fine.dtype == np.int32 and np.array_equal(fine, want) and np.array_equal(sub.fine_shifts_device().cpu().numpy(), want)
    assert np.array_equal(sub.shifts(), pk) and np.array_equal(whole.shifts(), pk)          # shifts() stays the whole-pixel pick
    assert np.array_equal(out_s, sref.apply_sub(frames, want, 0)) and np.array_equal(out_w, ref.apply(frames, pk, 0))
    assert sub.valid() == sref.valid_fine(want, (H, W))
    truth = np.array([(-16 * oy, -16 * ox) for oy, ox in OFFSETS])
    err = np.abs(fine - truth).max(axis=1)
    t64 = tmpl[m:-m, m:-m].astype(np.int64)
    d_s = ((out_s[:, m:-m, m:-m].astype(np.int64) - t64) ** 2).sum(axis=(1, 2))
    d_w = ((out_w[:, m:-m, m:-m].astype(np.int64) - t64) ** 2).sum(axis=(1, 2))
    print('error in sixteenths', err, 'squared difference whole / sub', np.round(d_w / np.maximum(d_s, 1), 1))
    assert (err <= 3).all(), err
    assert (d_s < d_w).all(), (d_s, d_w)


# ---- chunking, resident frames, consumers ---------------------------------------------------------------------------------------
S_, D_, BLOCKS = 3, 2, (2, 3)


@pytest.fixture(scope='module')
def moving():
    """33 uint16 frames of the scene, raised so that its values straddle 32768 (the interpolation must be told the signedness), at
    random sub-pixel offsets with a shear along y and a little noise; the ORACLE's fine shifts and corrected frames, rigid and in
    2 x 3 blocks: shared, never changed."""
    rs = np.random.RandomState(33)
    T, H, W = 33, 40, 48
    tmpl = scene(H, W, 0, 0, base=33000.0)
    frames = np.zeros((T, H, W), np.uint16)
    for t in range(T):
        oy, ox = rs.uniform(-2.4, 2.4, size=2)
        shear = rs.uniform(-0.6, 0.6) * (np.arange(H)[:, None] - H / 2) / H
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        y, x = y + oy, x + ox + shear
        v = 33000.0 + 3000 * np.sin(y / 5.3 + 0.3) * np.cos(x / 4.1) + 2000 * np.sin((y + x) / 7.7) + 1500 * np.cos(y / 3.1 - x / 6.3)
        frames[t] = np.rint(v + rs.randint(-20, 21, size=(H, W))).astype(np.uint16)
    assert frames.min() < 32768 < frames.max()
    sc = ref.scores(frames, tmpl, S_)
    pk = ref.pick(sc)
    fine = sref.refine(sc, pk)
    bsc = bref.block_scores(frames, tmpl, S_, D_, BLOCKS[0], BLOCKS[1], pk)
    bs, _ = bref.block_pick(bsc, pk, S_)
    bfine = sref.block_refine(bsc, pk, bs, S_)
    assert (fine % 16 != 0).any(axis=1).mean() > 0.8 and (bfine != fine[:, None, None, :]).any(-1).sum() > 30
    return dict(tmpl=tmpl, frames=frames, pk=pk, fine=fine, out=sref.apply_sub(frames, fine, 0),
                bs=bs, bfine=bfine, bout=sref.warp_sub(frames, bfine, 0))


@pytest.mark.parametrize('blocks', [None, BLOCKS])
def test_chunking_and_resident_frames_never_change_a_bit(moving, blocks):
    from deep_calcium_amd import MotionCorrector
    frames, tmpl = moving['frames'], moving['tmpl']
    T, H, W = frames.shape
    want_fine, want = (moving['fine'], moving['out']) if blocks is None else (moving['bfine'], moving['bout'])

    def run(parts, chunk_frames=None, device=False):
        mc = MotionCorrector((H, W), T, np.uint16, tmpl, max_shift=S_, chunk_frames=chunk_frames, blocks=blocks, max_dev=D_, subpixel=True)
        outs, a = [], 0
        for n in parts:
            piece = frames[a:a + n]
            outs.append(mc.feed(_dev(piece) if device else piece))
            a += n
        assert np.array_equal(mc.shifts(), moving['pk']) and (blocks is None or np.array_equal(mc.block_shifts(), moving['bs']))
        assert mc.valid() == sref.valid_fine(want_fine, (H, W))
        return mc.fine_shifts(), torch.cat(outs).cpu().numpy().view(np.uint16)
    for parts, cf, device in (((33,), None, False), ((1,) * 33, None, False), ((7, 7, 7, 7, 5), None, False), ((33,), 7, False),
                              ((33,), 1, False), ((33,), None, True), ((1,) * 33, None, True), ((7, 7, 7, 7, 5), 5, True)):
        fine, out = run(parts, cf, device)
        assert fine.shape == want_fine.shape and np.array_equal(fine, want_fine), (parts, cf, device)
        assert np.array_equal(out, want), (parts, cf, device)
    # correct=False only estimates
    mc = MotionCorrector((H, W), T, np.uint16, tmpl, max_shift=S_, blocks=blocks, max_dev=D_, subpixel=True)
    assert mc.feed(frames, correct=False) is None and np.array_equal(mc.fine_shifts(), want_fine)


@pytest.mark.parametrize('blocks', [None, BLOCKS])
def test_summarizer_takes_fine_shifts(moving, blocks):
    from deep_calcium_amd import MotionCorrector, SeriesSummarizer
    frames, tmpl = moving['frames'], moving['tmpl']
    T, H, W = frames.shape
    want_fine, want_out = (moving['fine'], moving['out']) if blocks is None else (moving['bfine'], moving['bout'])
    kinds = ('mean', 'std', 'corr')

    def summaries(feed, **kw):
        summ = SeriesSummarizer((H, W), T, np.uint16, kinds=kinds, **kw)
        for a in range(0, T, 8):
            summ.feed(feed(a, a + 8))
        return [summ.result(k) for k in kinds]
    mc = MotionCorrector((H, W), T, np.uint16, tmpl, max_shift=S_, blocks=blocks, max_dev=D_, subpixel=True)
    want = summaries(lambda a, b: mc.feed(frames[a:b]))                                   # fed the corrector's own output
    assert np.array_equal(mc.fine_shifts(), want_fine)
    from_oracle = summaries(lambda a, b: want_out[a:b])
    raw = lambda a, b: frames[a:b]                                                       # noqa: E731
    for got in (summaries(raw, fine_shifts=want_fine), summaries(raw, fine_shifts=want_fine.astype(np.int64), chunk_frames=5),
                summaries(raw, fine_shifts=mc.fine_shifts_device()), summaries(lambda a, b: _dev(frames[a:b]), fine_shifts=want_fine, chunk_frames=3)):
        for g, w, o in zip(got, want, from_oracle):
            assert g.dtype == np.float32 and np.array_equal(g.view(np.uint32), w.view(np.uint32)) and np.array_equal(w.view(np.uint32), o.view(np.uint32))
    assert not np.array_equal(summaries(raw)[0], want[0])
    assert not np.array_equal(summaries(raw, shifts=moving['pk'] if blocks is None else moving['bs'])[0], want[0])


@pytest.mark.parametrize('blocks', [None, BLOCKS])
def test_trace_extractor_takes_fine_shifts(moving, blocks):
    from deep_calcium_amd import MotionCorrector, RoiTraceExtractor
    frames, tmpl = moving['frames'], moving['tmpl']
    T, H, W = frames.shape
    want_fine, want_out = (moving['fine'], moving['out']) if blocks is None else (moving['bfine'], moving['bout'])
    rois = [np.argwhere(np.ones((5, 6), bool)) + (3, 4), np.argwhere(np.ones((H, W), bool)), np.array([[0, 0], [H - 1, W - 1]])]

    def sums(feed, **kw):
        ext = RoiTraceExtractor((H, W), T, np.uint16, rois, **kw)
        for a in range(0, T, 8):
            ext.feed(feed(a, a + 8))
        return ext.result('sum'), ext.result('zscore')
    mc = MotionCorrector((H, W), T, np.uint16, tmpl, max_shift=S_, blocks=blocks, max_dev=D_, subpixel=True)
    want = sums(lambda a, b: mc.feed(frames[a:b]))
    assert np.array_equal(want[0], np.stack([want_out.astype(np.int64)[:, r[:, 0], r[:, 1]].sum(1) for r in rois]))
    raw = lambda a, b: frames[a:b]                                                       # noqa: E731
    for got in (sums(raw, fine_shifts=want_fine), sums(raw, fine_shifts=mc.fine_shifts_device(), chunk_frames=5),
                sums(lambda a, b: _dev(frames[a:b]), fine_shifts=want_fine, chunk_frames=3)):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
    assert not np.array_equal(sums(raw)[0], want[0])


def test_estimate_fine_shifts_on_a_dataset_file(tmp_path, moving):
    from deep_calcium_amd import estimate_shifts_device, extract_traces_device, hdf5_min, summarize_series_device
    frames, tmpl = moving['frames'], moving['tmpl']
    T, H, W = frames.shape
    path, cpath = str(tmp_path / 'moving.hdf5'), str(tmp_path / 'corrected.hdf5')
    for p, data in ((path, frames), (cpath, moving['out'])):
        w = hdf5_min.Writer()
        w.create_dataset('series/raw', data=data)
        w.save(p)
    for cf in (None, 7):
        fine, t = estimate_shifts_device(path, template=tmpl, max_shift=S_, chunk_frames=cf, subpixel=True)
        assert fine.dtype == np.int32 and fine.shape == (T, 2) and np.array_equal(fine, moving['fine'])
        bfine, t = estimate_shifts_device(path, template=tmpl, max_shift=S_, chunk_frames=cf, blocks=BLOCKS, max_dev=D_, subpixel=True)
        assert bfine.dtype == np.int32 and bfine.shape == (T,) + BLOCKS + (2,) and np.array_equal(bfine, moving['bfine'])
    whole, _ = estimate_shifts_device(path, template=tmpl, max_shift=S_)                  # the default: the whole-pixel table it was
    assert np.array_equal(whole, moving['pk'])
    # the template is still built from whole-pixel corrections
    fine2, t2 = estimate_shifts_device(path, max_shift=S_, template_frames=10, subpixel=True)
    want_t = ref.make_template(frames[:10], S_, 1)
    sc = ref.scores(frames, want_t, S_)
    assert np.array_equal(t2, want_t) and np.array_equal(fine2, sref.refine(sc, ref.pick(sc)))
    # and the one-call functions take the fine shifts
    a = summarize_series_device(path, kind='std', fine_shifts=moving['fine'])
    b = summarize_series_device(cpath, kind='std')
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    mask = np.zeros((H, W), np.uint8)
    mask[5:12, 7:15] = 1
    mask[20:30, 30:41] = 1
    a = extract_traces_device(path, mask, kind='sum', fine_shifts=moving['fine'])
    b = extract_traces_device(cpath, mask, kind='sum')
    assert np.array_equal(a, b) and not np.array_equal(a, extract_traces_device(path, mask, kind='sum'))
