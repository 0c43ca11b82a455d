"""The pass every one-call function makes over a dataset file (deep_calcium_amd._reader._read_recording): each function, on each
path it offers -- plain, bin_frames, keep, keep + bin_frames --, equals the same reader class fed by hand, in ONE feed(), the frames
numpy makes on the host: moved by the shifts (fill 0; tests/_motion_ref.py), the dropped frames left out, the bins formed by
floor((2 s + b) / (2 b)) (tests/_tbin_ref.py).  Every comparison is equality.

The recording is 37 frames of 9 x 11 and chunk_frames = 5, so chunk ends fall inside bins (b = 3) and inside detrend segments; keep
drops frames 4 and 5, which straddle a chunk end, and 10..14, a whole chunk: a feed that keeps nothing."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _motion_ref as mref            # noqa: E402
import _tbin_ref as tref              # noqa: E402

T, H, W = 37, 9, 11
CHUNK, BIN, DETREND = 5, 3, 4
ROIS = [np.argwhere(np.ones((3, 4), bool)) + [1, 1], np.argwhere(np.ones((3, 3), bool)) + [5, 6], np.argwhere(np.ones((4, 2), bool)) + [1, 5]]
PATHS = ('plain', 'bin', 'keep', 'keep+bin')


@pytest.fixture(scope='module')
def rec(tmp_path_factory):
    """The dataset file, the corrections, and per path (the keywords of the one-call function, the frames that reach the reader)."""
    rs = np.random.RandomState(11)
    base = rs.randint(100, 1200, size=(1, H, W))
    raw = (base + rs.randint(-300, 600, size=(T, H, W))).astype(np.int16)                # some pixels go negative
    shifts = rs.randint(-2, 3, size=(T, 2)).astype(np.int32)
    keep = np.ones(T, bool)
    keep[[4, 5]] = False
    keep[10:15] = False
    path = str(tmp_path_factory.mktemp('driver') / 'recording.npz')
    np.savez(path, series_raw=raw)
    moved = mref.apply(raw, shifts, 0)
    frames = {'plain': moved, 'bin': tref.bin_time(moved, BIN), 'keep': moved[keep], 'keep+bin': tref.bin_time(moved[keep], BIN)}
    assert [len(frames[p]) for p in PATHS] == [37, 12, 30, 10]
    kws = {'plain': {}, 'bin': dict(bin_frames=BIN), 'keep': dict(keep=keep), 'keep+bin': dict(keep=keep, bin_frames=BIN)}
    for f in frames.values():
        f.setflags(write=False)
    return dict(path=path, raw=raw, shifts=shifts, kws=kws, frames=frames)


def _same(got, want):
    """Equality of results that are arrays, or tuples and lists of them."""
    if isinstance(want, (tuple, list)):
        assert isinstance(got, (tuple, list)) and len(got) == len(want)
        for g, w in zip(got, want):
            _same(g, w)
    elif want is None:
        assert got is None
    else:
        got, want = np.asarray(got), np.asarray(want)
        assert got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize('path', PATHS)
def test_summarize_series_device_equals_a_summarizer_fed_by_hand(rec, path):
    from deep_calcium_amd import SeriesSummarizer, summarize_series_device
    frames = rec['frames'][path]
    got = summarize_series_device(rec['path'], kind='corr', chunk_frames=CHUNK, shifts=rec['shifts'], detrend_frames=DETREND, **rec['kws'][path])
    summ = SeriesSummarizer((H, W), len(frames), np.int16, kinds=('corr',), detrend_frames=DETREND).feed(frames)
    _same(got, summ.result('corr', standardize=True))
    assert got.dtype == np.float32 and got.shape == (H, W) and np.isfinite(got).all() and got.std() > 0


@pytest.mark.parametrize('path', PATHS)
def test_roi_footprints_device_equals_footprints_fed_by_hand(rec, path):
    from deep_calcium_amd import RoiFootprints, roi_footprints_device
    frames = rec['frames'][path]
    got = roi_footprints_device(rec['path'], ROIS, halo=1, chunk_frames=CHUNK, shifts=rec['shifts'], detrend_frames=DETREND, **rec['kws'][path])
    fp = RoiFootprints((H, W), len(frames), np.int16, ROIS, halo=1, detrend_frames=DETREND).feed(frames)
    _same(got, (fp.result('corr'), fp.support(), fp.inside()))
    assert len(got[0]) == len(ROIS) and all(np.abs(c).max() > 0 for c in got[0])


@pytest.mark.parametrize('path', PATHS)
def test_roi_pair_corr_device_equals_pair_corr_fed_by_hand(rec, path):
    from deep_calcium_amd import RoiPairCorr, roi_pair_corr_device
    frames = rec['frames'][path]
    got = roi_pair_corr_device(rec['path'], ROIS, chunk_frames=CHUNK, shifts=rec['shifts'], detrend_frames=DETREND, **rec['kws'][path])
    pc = RoiPairCorr((H, W), len(frames), np.int16, ROIS, detrend_frames=DETREND).feed(frames)
    _same(got, (pc.result('corr'), pc.pixels()))
    assert [c.shape for c in got[0]] == [(12, 12), (9, 9), (8, 8)] and all(np.abs(c).max() > 0 for c in got[0])


def test_extract_traces_device_equals_an_extractor_fed_by_hand(rec):
    from deep_calcium_amd import RoiTraceExtractor, extract_traces_device
    frames = rec['frames']['plain']
    ext = RoiTraceExtractor((H, W), T, np.int16, ROIS).feed(frames)
    for kind in ('sum', 'mean', 'zscore'):
        _same(extract_traces_device(rec['path'], ROIS, kind=kind, chunk_frames=CHUNK, shifts=rec['shifts']), ext.result(kind))
    want = np.stack([frames[:, r[:, 0], r[:, 1]].astype(np.int64).sum(1) for r in ROIS])
    assert np.array_equal(ext.result('sum'), want)


def test_frame_quality_device_equals_frame_quality_fed_by_hand(rec):
    from deep_calcium_amd import FrameQuality, frame_quality_device
    frames = rec['frames']['plain']
    tmpl, rect = mref.rounded_mean(frames), ((1, 8), (2, 9))
    fq = FrameQuality((H, W), T, np.int16, template=tmpl, rect=rect).feed(frames)
    got = frame_quality_device(rec['path'], template=tmpl, rect=rect, chunk_frames=CHUNK, shifts=rec['shifts'])
    _same(got, (fq.result('mean'), fq.result('corr')))
    fq = FrameQuality((H, W), T, np.int16).feed(frames)
    _same(frame_quality_device(rec['path'], chunk_frames=CHUNK, shifts=rec['shifts']), (fq.result('mean'), None))
    assert np.array_equal(fq.result('moments')[:, 0], frames.astype(np.int64).sum((1, 2)))


def test_dff_traces_device_equals_an_extractor_and_a_baseline_fed_by_hand(rec):
    from deep_calcium_amd import RoiTraceExtractor, TraceBaseline, dff_traces_device, neuropil_rois
    frames = rec['frames']['plain']
    rings = neuropil_rois(ROIS, (H, W), 1, 3)
    assert all(len(r) for r in rings)
    ext = RoiTraceExtractor((H, W), T, np.int16, ROIS + rings).feed(frames)          # the ROIs followed by their rings, as the one call lists them
    sums, R = ext.sums_device(), len(ROIS)
    for kind in ('dff', 'num'):
        tb = TraceBaseline(sums[:R], [len(r) for r in ROIS], 9, neuropil_sums=sums[R:], neuropil_areas=[len(r) for r in rings], weight=0.7)
        _same(dff_traces_device(rec['path'], ROIS, 9, kind=kind, neuropil=(1, 3, 0.7), chunk_frames=CHUNK, shifts=rec['shifts']), tb.result(kind))
    tb = TraceBaseline(sums[:R], [len(r) for r in ROIS], 9)
    _same(dff_traces_device(rec['path'], ROIS, 9, chunk_frames=CHUNK, shifts=rec['shifts']), tb.result('dff'))
