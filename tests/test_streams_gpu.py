"""Every recording reader, trace stage and one-call chain OFF the default stream (helpers and the stage table: tests/_streams.py).

The rest of the suite pins the arithmetic of these stages bit for bit -- on the default stream, where every launch is ordered
whether or not the code ordered it.  Here the reference is that default-stream run, and the same stage must give the same bits

  1. fed on a fresh non-blocking side stream that a hold keeps busy while the host enqueues everything behind it: a launch that
     dropped its stream argument, a hipMemsetAsync or copy on the null stream, a wrong wait or record of the two-slot upload runs
     ahead of its neighbours and reads stale values;
  2. constructed under one stream with every fill of its constructor held back, and fed under another with no synchronisation in
     between: a reader must order its feed() after its own constructor.

A held run proves that its hold held: an event recorded on the held stream directly after the last launch must not have happened
yet ("hold too short" otherwise), and the hold's measured length covers four times the measured enqueue.  DC_STREAM_HOLDS=0 in
the environment runs the same file with every hold a no-op.  test_a_launch_on_the_wrong_stream_changes_the_result shows that the
method sees what it claims to see.
"""
import json
import os
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _streams as st           # noqa: E402


@pytest.fixture(scope='module')
def L(dclib):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    st._units_per_ms(torch)               # the hold's calibration, outside every timed region
    torch.cuda.synchronize()
    yield dclib
    torch.cuda.synchronize()
    path = os.environ.get('DC_STREAM_LOG')            # the measured enqueue times and hold lengths, for whoever asks
    if path:
        with open(path, 'w') as fp:
            json.dump(st.LOG, fp, indent=1)


_REFERENCE = {}


def _reference(case, kind, dtype):
    """The default-stream run, once per case and dtype (readers: resident frames; matrix stages: numpy input), never changed."""
    key = (case.id, np.dtype(dtype).name)
    if key not in _REFERENCE:
        _REFERENCE[key] = st.reference(case, st.data_of(kind, dtype, 0, 'device' if kind == 'recording' else 'numpy'))
    return _REFERENCE[key]


# ---- the method sees what it claims to see ----------------------------------------------------------------------------------
def test_a_launch_on_the_wrong_stream_changes_the_result(L):
    """dc_fill(3) then dc_scale_flat(2) on a buffer of ones, through the raw C ABI.  Both on the held stream: 6 everywhere.  The
    second on the null stream instead: it does not wait for the side stream (non-blocking), doubles the ones first and the fill
    lands last -- 3, not 6.  Without this the equalities below would prove nothing."""
    n = 4099
    S = torch.cuda.Stream()
    want = np.full(n, 6.0, np.float32)
    for second_on_null in (False, True):
        buf = torch.ones(n, dtype=torch.float32, device='cuda')
        torch.cuda.synchronize()
        h = st.hold(S, st.MIN_HOLD_MS)
        L.dc_fill(buf.data_ptr(), n, 3.0, S.cuda_stream)
        L.dc_scale_flat(buf.data_ptr(), n, 2.0, None if second_on_null else S.cuda_stream)
        probe = st.Probe(S, [h] if h is not None else [])
        probe.mark()
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        if not second_on_null:
            assert np.array_equal(got, want)
        elif h is not None:
            assert probe.busy, 'hold too short (%.2f ms)' % h.ms()
            assert np.array_equal(got, np.full(n, 3.0, np.float32)), got[:4]


# ---- regime 1: a held side stream -------------------------------------------------------------------------------------------
_READERS, _READER_IDS = st.params(st.READERS, ('device', 'numpy'))
_MATRIX, _MATRIX_IDS = st.params(st.MATRIX, ('numpy', 'resident'))


@pytest.mark.parametrize('case,dtype,mode', _READERS, ids=_READER_IDS)
def test_reader_on_a_held_side_stream(L, case, dtype, mode):
    """Constructed on the default stream, fed under a held side stream -- resident frames (the whole feed is enqueued behind the
    hold) and numpy frames in six chunks (the hold is checked after the first two; then both pinned and both device slots wrap and
    the hand-back events of the two-slot upload carry the order) -- every result equals the default-stream run in every bit."""
    want = _reference(case, 'recording', dtype)
    what = 'held %s-%s-%s' % (case.id, np.dtype(dtype).name, mode)
    got = st.held_side_stream(case, st.data_of('recording', dtype, 0, mode), st.data_of('recording', dtype, 1, mode), what)
    st.same(got, want, what)


@pytest.mark.parametrize('case,dtype,mode', _MATRIX, ids=_MATRIX_IDS)
def test_matrix_stage_on_a_held_side_stream(L, case, dtype, mode):
    """Constructed on the default stream from numpy or from the test's own resident matrix, every kind of result_device() taken
    under a held side stream: the bits of the default-stream run."""
    want = _reference(case, 'matrix', dtype)
    what = 'held %s-%s-%s' % (case.id, np.dtype(dtype).name, mode)
    got = st.held_side_stream(case, st.data_of('matrix', dtype, 0, mode), st.data_of('matrix', dtype, 1, mode), what)
    st.same(got, want, what)


# ---- regime 2: delayed constructor fills ------------------------------------------------------------------------------------
_DELAYED, _DELAYED_IDS = st.params(st.READERS, ('device',), only=lambda c: c.init is not None)


@pytest.mark.parametrize('case,dtype,mode', _DELAYED, ids=_DELAYED_IDS)
def test_reader_fed_on_another_stream_than_its_constructor(L, case, dtype, mode):
    """Constructed under stream A with a hold in front of every torch.zeros / torch.full of the constructor, fed under stream B
    without any synchronisation by the test: feed() waits for the event the constructor recorded, so no fill lands on a chunk's
    contribution.  Delaying only the fills (and, for FrameQuality, the one kernel) is safe, stage by stage, read from the
    constructors:
      SeriesSummarizer (detrend)  no index tables; _pvar, _pcov, _sum_total (zeros) and _vmax_total (full) come last.
      MotionCorrector             the template is uploaded from numpy, which blocks the host, before the first fill; _shifts,
                                  _coarse, _bshifts, _fine are zeros, the binned template is a kernel behind them on the same stream.
      RoiFootprints, RoiPairCorr  the CSR rows, tiles and offsets of the owner and of its extractor are uploaded from numpy before
                                  the fills of _mom, _pxx, _pxs, _pss / _a, _g, _pooled.
      FrameQuality                no fill: the template's sums are a kernel, held back by one hold in front of the constructor;
                                  the template is the test's own resident tensor, so no upload waits that hold out.
    The other readers make their state with torch.empty and uploads from numpy only."""
    want = _reference(case, 'recording', dtype)
    what = 'delayed %s-%s' % (case.id, np.dtype(dtype).name)
    got = st.delayed_constructor(case, st.data_of('recording', dtype, 0, mode), st.data_of('recording', dtype, 1, mode), what)
    st.same(got, want, what)


# ---- the one-call chains ----------------------------------------------------------------------------------------------------
def _held_chain(monkeypatch, call, what):
    """call() with the caller's current stream, a side stream, held.  The chain constructs its reader on that stream, and the
    uploads of a constructor wait a hold out, so the hold goes in where the chain feeds its first chunk; it is checked where the
    recording has been fed and the sums are handed on in place, on entry to TraceBaseline.from_stacked (the copy of the result
    back to the host blocks until the stream has run dry)."""
    from deep_calcium_amd import _reader, dff
    want = call()
    S = torch.cuda.Stream()
    feed, from_stacked = _reader._FrameReader.feed, dff.TraceBaseline.from_stacked.__func__
    state = {}

    def held_feed(self, frames):
        if 't0' not in state:
            h = st.hold(S, state['ms']) if state['ms'] is not None else None
            if h is not None:
                state['holds'].append(h)
            state['t0'] = time.perf_counter()
        return feed(self, frames)

    def marked(cls, *args, **kw):
        state['probe'].mark()
        return from_stacked(cls, *args, **kw)
    monkeypatch.setattr(_reader._FrameReader, 'feed', held_feed)
    monkeypatch.setattr(dff.TraceBaseline, 'from_stacked', classmethod(marked))
    with torch.cuda.stream(S):
        state.update(ms=None, holds=[], probe=st.Probe(S, []))
        call()
        unheld_s = state['probe'].t - state.pop('t0')
        S.synchronize()
        holds = []
        state.update(ms=st.hold_ms(unheld_s), holds=holds, probe=st.Probe(S, holds))
        got = call()
    S.synchronize()
    st._finish(what, state['probe'], holds, state['t0'], unheld_s)
    return got, want


def _recording_file(tmp_path, dtype):
    from deep_calcium_amd import hdf5_min
    rec = st.data_of('recording', dtype, 0, 'numpy')
    path = str(tmp_path / 'rec.hdf5')
    w = hdf5_min.Writer()
    w.create_dataset('series/raw', data=rec.frames)
    w.save(path)
    return path


@pytest.mark.parametrize('dtype', st.DTYPES, ids=lambda d: np.dtype(d).name)
def test_dff_chain_on_a_held_stream(L, tmp_path, monkeypatch, dtype):
    """dff_traces_device with the caller's current stream held: extractor, combine, baseline and scale hand device tensors on in
    place on that one stream.  Four chunks of numpy frames, so the host is not blocked before the sums are handed on."""
    from deep_calcium_amd.dff import dff_traces_device
    path = _recording_file(tmp_path, dtype)
    got, want = _held_chain(monkeypatch, lambda: dff_traces_device(path, st.ROIS, 11, percentile=20, neuropil=(1, 4, 0.7), offset=400,
                                                                   chunk_frames=10, shifts=st.data_of('recording', dtype, 0, 'numpy').shifts),
                            'held dff chain %s' % np.dtype(dtype).name)
    st.same(dict(dff=got), dict(dff=want), 'dff chain')


@pytest.mark.parametrize('dtype', st.DTYPES, ids=lambda d: np.dtype(d).name)
def test_deconvolution_chain_on_a_held_stream(L, tmp_path, monkeypatch, dtype):
    """deconvolve_traces_device likewise: the dF/F chain behind the hold, then the noise-constrained search with a fitted baseline
    on the same side stream."""
    from deep_calcium_amd.deconv import deconvolve_traces_device
    path = _recording_file(tmp_path, dtype)
    got, want = _held_chain(monkeypatch, lambda: deconvolve_traces_device(path, st.ROIS, 11, tau=0.5, fps=16.0, k='noise', baseline='fit',
                                                                          percentile=20, offset=400, chunk_frames=10),
                            'held deconvolution chain %s' % np.dtype(dtype).name)
    st.same(dict(calcium=got[0], spikes=got[1]), dict(calcium=want[0], spikes=want[1]), 'deconvolution chain')
