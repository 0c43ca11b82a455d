"""Temporal binning on the device (include/dcunet.h dc_series_bin_time; TemporalBinner; bin_frames= of summarize_series_device,
roi_footprints_device, roi_pair_corr_device and split_rois_device) against the integer oracle of tests/_tbin_ref.py.  Every
comparison is equality; every output buffer is pre-filled with a pattern and has a guard on both sides."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _bidi_ref as bref              # noqa: E402
import _gridcaps as caps              # noqa: E402
import _motion_ref as mref            # noqa: E402
import _pair_ref as pref              # noqa: E402
import _tbin_ref as ref               # noqa: E402

DTYPES = [np.int16, np.uint16]
PATTERN, GARBAGE = 0x5a5a, 0x7b7b7b7b
X_CAP = 4096 * 256                    # groups of 8 pixels one trip of the x grid covers (kBinBlocksX workgroups of 256 threads)
SLOT_CAP = caps.FRAME_CAP             # output slots one trip of the y grid covers


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).cuda()


def _rand(rs, shape, dtype):
    info = np.iinfo(dtype)
    return rs.randint(info.min, info.max + 1, size=shape).astype(dtype)


def _bin(L, chunk, b, phase, carry_in=None, odd=0, odd_out=0, odd_carry=0):
    """One dc_series_bin_time call.  out: a buffer of 0x5a5a with a guard on both sides; carry: int32 with a guard on both sides,
    holding carry_in (phase > 0) or garbage (phase == 0: it must not be read).  odd / odd_out: frames / out start that many
    elements into their 16-byte aligned allocation; odd_carry: carry starts that many int32 past a 16-byte boundary.
    -> (out (n_out,H,W), carry (H,W) int32 after the call)."""
    tc, H, W = chunk.shape
    hw = H * W
    n_out, rem = (phase + tc) // b, (phase + tc) % b
    src = torch.zeros((chunk.size + odd + 8,), dtype=torch.int16, device='cuda')
    src[odd:odd + chunk.size] = _dev(chunk).reshape(-1)
    lead = 8 + odd_out
    buf = torch.full((lead + n_out * hw + 8,), PATTERN, dtype=torch.int16, device='cuda')
    clead = 4 + odd_carry
    before = np.full(clead + hw + 4, GARBAGE, np.int32)
    if phase > 0:
        before[clead:clead + hw] = np.asarray(carry_in, np.int64).reshape(-1)
    cbuf = torch.from_numpy(before.copy()).cuda()
    assert src.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0 and cbuf.data_ptr() % 16 == 0
    L.dc_series_bin_time(src.data_ptr() + 2 * odd, int(chunk.dtype == np.uint16), tc, H, W, b, phase, cbuf.data_ptr() + 4 * clead,
                         buf.data_ptr() + 2 * lead, _st())
    got, cgot = buf.cpu().numpy(), cbuf.cpu().numpy()
    assert (got[:lead] == PATTERN).all() and (got[lead + n_out * hw:] == PATTERN).all()          # nothing around `out` is written
    assert (cgot[:clead] == GARBAGE).all() and (cgot[clead + hw:] == GARBAGE).all()              # nor around carry
    if rem == 0:
        assert np.array_equal(cgot, before)                                                      # a call that leaves no bin open leaves carry alone
    return got[lead:lead + n_out * hw].reshape(n_out, H, W).view(chunk.dtype), cgot[clead:clead + hw].reshape(H, W)


def _cases(b):
    """(phase, tc): whole bins from an empty carry; the frame that closes a bin and leaves none open; a call that closes none;
    several bins between a carried head and an open tail (carry is read and written by one call: the write must not reach the
    read, whichever workgroup runs first)."""
    cases = [(0, 2 * b), (b - 1, 1)]
    if b >= 2:
        cases += [(0, b - 1), (b // 2, 3 * b + 1)]
    if b >= 3:
        cases += [(1, b - 2)]
    return cases


# ---- dc_series_bin_time ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('b', [1, 2, 3, 7, 64])
@pytest.mark.parametrize('dtype', DTYPES)
def test_bin_time_equals_the_oracle(dclib, b, dtype):
    rs = np.random.RandomState(10 * b + int(dtype == np.uint16))
    info = np.iinfo(dtype)
    for H in (1, 3):
        for W in (1, 7, 8, 19, 517):
            for phase, tc in _cases(b):
                whole = _rand(rs, (phase + tc, H, W), dtype)
                flat = whole.reshape(phase + tc, H * W)                                 # a view
                flat[:, 0] = info.min                                                   # a bin of nothing but the smallest value
                if H * W > 1:
                    flat[:, -1] = info.max                                              # and one of the largest
                if H * W > 2:
                    flat[0::2, 1], flat[1::2, 1] = info.min, info.max                   # and the two in turn
                prev, chunk = whole[:phase], whole[phase:]
                carry_in = prev.astype(np.int64).sum(0)
                want, want_carry, rem = ref.stream(chunk, b, phase, carry_in)
                if phase + tc >= b:
                    assert np.array_equal(want[:1], ref.bin_time(whole, b)[:1])
                offsets = ((0, 0, 0), (1, 0, 0), (0, 1, 1), (3, 5, 2)) if W in (8, 19) or b == 3 else ((0, 0, 0), (1, 1, 1))
                for odd, odd_out, odd_carry in offsets:
                    got, carry = _bin(dclib, chunk, b, phase, carry_in, odd, odd_out, odd_carry)
                    where = (H, W, phase, tc, odd, odd_out, odd_carry)
                    assert got.shape[0] == (phase + tc) // b and np.array_equal(got, want), where
                    if rem > 0:
                        assert np.array_equal(carry, want_carry), where
                    if b == 1:
                        assert np.array_equal(got, chunk), where                        # a copy


def test_carry_is_read_before_the_same_call_writes_it(dclib):
    """phase > 0, bins closed and a bin left open: slot 0 reads the carry the open slot overwrites.  Which workgroup runs first is
    not up to the kernel, so the case is repeated, at the shapes at which a write that overtook the read was once seen (one
    workgroup per slot) and at one of several workgroups per slot."""
    rs = np.random.RandomState(8)
    for H, W, b, phase, tc, reps in ((3, 8, 3, 1, 10, 40), (1, 19, 2, 1, 4, 20), (40, 520, 4, 3, 11, 10)):
        for _ in range(reps):
            whole = _rand(rs, (phase + tc, H, W), np.uint16)
            carry_in = whole[:phase].astype(np.int64).sum(0)
            want, want_carry, rem = ref.stream(whole[phase:], b, phase, carry_in)
            assert rem > 0 and want.shape[0] >= 1
            got, carry = _bin(dclib, whole[phase:], b, phase, carry_in)
            assert np.array_equal(got, want) and np.array_equal(carry, want_carry), (H, W, b)


@pytest.mark.parametrize('dtype', DTYPES)
def test_bin_time_of_the_extreme_bins(dclib, dtype):
    info = np.iinfo(dtype)
    for H, W in ((1, 1), (1, 9), (2, 8)):
        for v in (info.min, info.max):
            f = np.full((128, H, W), v, dtype)
            for b in (64, 63, 5):
                got, _ = _bin(dclib, f, b, 0)
                assert got.shape[0] == 128 // b and (got == v).all(), (H, W, v, b)
    if dtype == np.int16:
        f = np.array([-1, -2, -2, -3, 1, 2], np.int16).reshape(6, 1, 1)
        assert _bin(dclib, f, 2, 0)[0].reshape(-1).tolist() == [-1, -2, 2]              # the mean rounds half UP, below zero too


def test_bin_time_of_no_frame_launches_nothing_and_bad_arguments_are_refused(dclib):
    from deep_calcium_amd._lib import DcunetError
    buf = torch.full((256,), PATTERN, dtype=torch.int16, device='cuda')
    carry = torch.full((64,), GARBAGE, dtype=torch.int32, device='cuda')
    fr = torch.zeros((256,), dtype=torch.int16, device='cuda')
    assert dclib.dc_series_bin_time(fr.data_ptr(), 0, 0, 3, 5, 4, 2, carry.data_ptr(), buf.data_ptr(), _st()) == 0
    for kw in (dict(b=0), dict(b=65), dict(phase=4), dict(phase=-1)):
        a = dict(dict(b=4, phase=0), **kw)
        with pytest.raises(DcunetError, match=r'\(%d\)' % (-3 if a['b'] > 64 else -1)):
            dclib.dc_series_bin_time(fr.data_ptr(), 0, 4, 3, 5, a['b'], a['phase'], carry.data_ptr(), buf.data_ptr(), _st())
    with pytest.raises(DcunetError, match=r'\(-1\).*out overlaps frames'):
        dclib.dc_series_bin_time(fr.data_ptr(), 0, 4, 3, 5, 2, 0, carry.data_ptr(), fr.data_ptr() + 2 * 59, _st())
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == PATTERN).all() and (carry.cpu().numpy() == GARBAGE).all()


def test_bin_time_past_the_x_cap(dclib):
    """One frame of more than 8 * 4096 * 256 values at b = 1: the last groups are reached on a second trip of the x grid."""
    H, W = caps.BIG_H, caps.BIG_W
    first = X_CAP * 8                                                                   # the first value of the second trip
    assert H * W > first and H * W - first < caps.BIG_BAND * W
    rs = np.random.RandomState(5)
    frames = _rand(rs, (1, H, W), np.int16)
    got, _ = _bin(dclib, frames, 1, 0)
    assert np.array_equal(got.reshape(-1)[first:first + 8], frames.reshape(-1)[first:first + 8])
    assert np.array_equal(got.reshape(-1)[first:], frames.reshape(-1)[first:]) and np.array_equal(got, frames)


@pytest.mark.parametrize('dtype', DTYPES)
def test_bin_time_past_the_slot_cap(dclib, dtype):
    """More output slots than the y grid holds, at 1 x 8: slot 65535 is the first of the second trip."""
    rs = np.random.RandomState(6)
    base = caps.base_frames(rs, (1, 8), dtype)
    n = caps.TWO_TRIPS
    assert caps.first_stride_trip(n, SLOT_CAP) == SLOT_CAP
    frames = caps.expand(base, n)
    got, _ = _bin(dclib, frames, 1, 0)
    assert np.array_equal(got[SLOT_CAP], frames[SLOT_CAP]) and np.array_equal(got, frames)
    # b = 2 with an open bin behind the last closed one: the open slot, too, is a second-trip slot
    frames = caps.expand(base, 2 * n + 1)
    want, want_carry, rem = ref.stream(frames, 2, 0, None)
    got, carry = _bin(dclib, frames, 2, 0)
    assert rem == 1 and want.shape[0] == n and np.array_equal(got[SLOT_CAP], want[SLOT_CAP]) and np.array_equal(got, want)
    assert np.array_equal(carry, want_carry)


# ---- TemporalBinner -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DTYPES)
def test_binner_is_chunking_invariant(dtype):
    from deep_calcium_amd import TemporalBinner
    rs = np.random.RandomState(12)
    T, H, W, b = 29, 5, 19, 4
    frames = _rand(rs, (T, H, W), dtype)
    want = ref.bin_time(frames, b)
    assert want.shape[0] == 7
    for step in (1, 3, 4, 5, 29):
        for resident in (False, True):
            tb = TemporalBinner((H, W), T, dtype, bin_frames=b, chunk_frames=4)
            outs = []
            for a in range(0, T, step):
                part = frames[a:a + step]
                out = tb.feed(_dev(part) if resident else part)
                assert out.dtype == torch.int16 and out.is_cuda and out.is_contiguous() and tuple(out.shape[1:]) == (H, W)
                assert out.shape[0] == (a % b + len(part)) // b
                outs.append(out)
            got = torch.cat(outs).cpu().numpy().view(dtype)
            assert np.array_equal(got, want), (step, resident)
            assert (tb.n_out, tb.fed, tb.emitted) == (7, 29, 7)                          # the tail of one frame is dropped
    with pytest.raises(ValueError, match='30 fed|after 29 fed'):
        tb.feed(frames[:1])


def test_binner_applies_the_corrections_before_the_sum():
    from deep_calcium_amd import TemporalBinner
    rs = np.random.RandomState(13)
    T, H, W, b, p = 17, 12, 21, 3, 2
    for dtype in DTYPES:
        frames = _rand(rs, (T, H, W), dtype)
        shifts = rs.randint(-3, 4, size=(T, 2)).astype(np.int32)
        lines = bref.apply(frames, p, 0)
        for kw, moved in ((dict(shifts=shifts, bidi=p), mref.apply(lines, shifts, 0)), (dict(bidi=p), lines),
                          (dict(shifts=shifts), mref.apply(frames, shifts, 0))):
            want = ref.bin_time(moved, b)
            assert not np.array_equal(want, ref.bin_time(frames, b))
            for resident in (False, True):
                tb = TemporalBinner((H, W), T, dtype, bin_frames=b, chunk_frames=4, **kw)
                outs = [tb.feed(_dev(frames[a:a + 5]) if resident else frames[a:a + 5]) for a in range(0, T, 5)]
                assert np.array_equal(torch.cat(outs).cpu().numpy().view(dtype), want), (sorted(kw), resident)
                assert tb.emitted == T // b


# ---- the one-call functions -------------------------------------------------------------------------------------------------------
def _rois():
    region = pref.scene('two', 3)[1]
    return [region, np.array([[0, x] for x in range(3, 14)], np.int64), np.array([[9, 1], [9, 2]], np.int64)]


def _same_lists(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x, y)


def test_one_call_functions_with_bin_frames(tmp_path):
    from deep_calcium_amd import (RoiFootprints, RoiPairCorr, SeriesSummarizer, roi_footprints_device, roi_pair_corr_device,
                                  summarize_series_device)
    T, b = 66, 4
    frames = pref.scene('two', 3, T=T)[0]
    H, W = frames.shape[1:]
    path = str(tmp_path / 'recording.npz')
    np.savez(path, series_raw=frames)
    binned = ref.bin_time(frames, b)
    assert binned.shape[0] == 16 and T % b == 2
    rois = _rois()
    # the summary of the oracle's binned frames
    for standardize in (True, False):
        want = SeriesSummarizer((H, W), T // b, np.int16, kinds=('corr',)).feed(binned).result('corr', standardize=standardize)
        got = summarize_series_device(path, kind='corr', standardize=standardize, bin_frames=b, chunk_frames=7)
        assert got.dtype == np.float32 and np.array_equal(got, want)
    assert not np.array_equal(summarize_series_device(path, kind='corr', bin_frames=b), summarize_series_device(path, kind='corr'))
    pc = RoiPairCorr((H, W), T // b, np.int16, rois).feed(binned)
    corr, pixels = roi_pair_corr_device(path, rois, bin_frames=b, chunk_frames=7)
    _same_lists(corr, pc.result('corr'))
    _same_lists(pixels, pc.pixels())
    fp = RoiFootprints((H, W), T // b, np.int16, rois).feed(binned)
    corr, coords, inside = roi_footprints_device(path, rois, bin_frames=b, chunk_frames=7)
    _same_lists(corr, fp.result('corr'))
    _same_lists(coords, fp.support())
    _same_lists(inside, fp.inside())
    # bin_frames = 1 is what None is
    for kind in ('mean', 'std', 'corr'):
        assert np.array_equal(summarize_series_device(path, kind=kind, bin_frames=1), summarize_series_device(path, kind=kind))
    _same_lists(roi_pair_corr_device(path, rois, bin_frames=1)[0], roi_pair_corr_device(path, rois)[0])
    _same_lists(roi_footprints_device(path, rois, bin_frames=1)[0], roi_footprints_device(path, rois)[0])
    # the corrections go in front of the sum
    rs = np.random.RandomState(2)
    shifts = rs.randint(-2, 3, size=(T, 2)).astype(np.int32)
    moved = ref.bin_time(mref.apply(bref.apply(frames, 1, 0), shifts, 0), b)
    want = SeriesSummarizer((H, W), T // b, np.int16, kinds=('corr',)).feed(moved).result('corr', standardize=True)
    assert np.array_equal(summarize_series_device(path, kind='corr', shifts=shifts, bidi=1, bin_frames=b), want)
    with pytest.raises(ValueError, match='bin_frames'):
        summarize_series_device(path, kind='corr', bin_frames=64 + 3)
    with pytest.raises(ValueError, match='bin_frames'):
        np.savez(str(tmp_path / 'short.npz'), series_raw=frames[:3])
        summarize_series_device(str(tmp_path / 'short.npz'), kind='corr', bin_frames=4)


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def test_binning_splits_what_single_frames_do_not(tmp_path):
    """The scene of tests/test_tbin_api.py (its conditions on the float64 oracle are asserted there): frame by frame the two
    cells stay one ROI, at bin_frames = 4 they are the two planted halves."""
    from deep_calcium_amd import split_rois_device
    frames, region, left, right, _ = pref.scene('two', 11, amplitude=40.0, sigma=40.0, T=1024)
    path = str(tmp_path / 'scene.npz')
    np.savez(path, series_raw=frames)
    new, origin, gaps = split_rois_device(path, [region], min_gap=0.1, min_area=8, iterations=16)
    assert origin == [0] and np.array_equal(new[0], region) and gaps[0] < 0.1
    new, origin, gaps = split_rois_device(path, [region], min_gap=0.1, min_area=8, iterations=16, bin_frames=4)
    assert origin == [0, 0] and np.array_equal(new[0], left) and np.array_equal(new[1], right) and gaps[0] >= 0.2
