"""Helpers of tests/test_streams_gpu.py: a bounded hold on a stream, the two regimes that run a stage behind one, and the stage
table the tests are parametrised over (tests/test_streams.py checks on the CPU that no public stage is missing from it).

On the default stream everything is ordered whether or not the code ordered it.  Here a stage is driven on a fresh side stream
that is kept busy with unrelated work -- hold() -- while the host enqueues all of the stage's launches behind it: a launch that
lost its stream argument, a memset or copy on the null stream, a missing event wait then runs AHEAD of its neighbours, reads stale
(but in-range) values and changes bits that the default-stream run of the same stage pins.

Importing this module needs numpy only; torch and the package are imported where a function needs them.
"""
import os
import time

import numpy as np

HOLDS = os.environ.get('DC_STREAM_HOLDS', '1') != '0'      # 0: every hold() is a no-op -- the first run of a new stage's cases
FACTOR = 4                            # a hold lasts at least this many times the measured host-side enqueue of what it holds back
MIN_HOLD_MS, MAX_HOLD_MS = 50.0, 2000.0           # the floor: a few hundred enqueues of these small stages, against host jitter
LOG = []                              # one dict per held run: the enqueue times and hold lengths (test_streams_gpu.py dumps it)

H, W, T, CHUNK = 24, 40, 40, 7        # the recording: 6 chunks of numpy frames, so both pinned and both device slots are reused
R, TM = 65, 257                       # the trace matrices: the ragged-tile shape of the deconvolution tests
DTYPES = (np.int16, np.uint16)


# ---- the hold -------------------------------------------------------------------------------------------------------------------
_RATE = {}


def _busy(torch, units):
    """`units` of bounded, unrelated work on the current stream: torch.cuda._sleep cycles, or rounds of a 2048^2 matmul chain."""
    if hasattr(torch.cuda, '_sleep'):
        torch.cuda._sleep(int(units))
        return
    junk = _RATE.setdefault('junk', torch.randn(2048, 2048, device='cuda') * 0.01)
    t = junk
    for _ in range(max(1, int(units))):
        t = (t @ junk) * 0.01


def _units_per_ms(torch):
    """How much _busy() work one millisecond is, measured once with two events around a probe that is then scaled to ~30 ms."""
    if 'rate' not in _RATE:
        units = 1000000 if hasattr(torch.cuda, '_sleep') else 4
        for _ in range(3):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _busy(torch, units)
            b.record()
            b.synchronize()
            rate = units / max(a.elapsed_time(b), 1e-3)
            units = max(1, int(30.0 * rate))
        _RATE['rate'] = rate
    return _RATE['rate']


class Hold(object):
    """What hold() enqueued: two timing events around the work; ms() once the stream has passed them."""

    def __init__(self, torch, stream, asked_ms):
        self.asked_ms = asked_ms
        units = 1.25 * asked_ms * _units_per_ms(torch)                   # a quarter more: the clock of the probe may have moved
        self._a, self._b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            self._a.record(stream)
            _busy(torch, units)
            self._b.record(stream)

    def over(self):
        return self._b.query()

    def ms(self):
        self._b.synchronize()
        return self._a.elapsed_time(self._b)


def hold(stream, ms, enabled=None):
    """Keeps `stream` busy for about `ms` milliseconds with bounded work nothing depends on (no kernel waits for the host) ->
    the Hold, or None where holds are disabled (enabled=False, or DC_STREAM_HOLDS=0 in the environment)."""
    import torch
    if not (HOLDS if enabled is None else enabled):
        return None
    return Hold(torch, stream, float(ms))


def hold_ms(enqueue_s):
    """The length of the hold in front of work whose unheld enqueue took `enqueue_s` seconds on the host."""
    return min(max(FACTOR * 1000.0 * enqueue_s, MIN_HOLD_MS), MAX_HOLD_MS)


class Probe(object):
    """mark(): called by a drive function directly after its last launch that does not block the host.  It notes the host time
    and, behind holds, whether they still hold: an event recorded on the held stream there must not have happened yet -- and, which
    is stricter, neither must the end of the last hold itself (launches still queued behind a hold that is over would keep the
    first from happening too)."""

    def __init__(self, stream, holds):
        self.stream, self.holds, self.t, self.busy = stream, holds, None, None

    def mark(self):
        import torch
        if self.t is not None:
            return
        self.t = time.perf_counter()
        ev = torch.cuda.Event()
        ev.record(self.stream)
        self.busy = not ev.query() and not (self.holds and self.holds[-1].over())


def _finish(what, probe, holds, t0, unheld_s):
    """After the streams were synchronised: the hold must have held, and its measured length covers FACTOR enqueues."""
    assert probe.t is not None, '%s: the drive function never called mark()' % what
    if not holds:
        return
    held_s = probe.t - t0
    measured = [h.ms() for h in holds]
    LOG.append(dict(case=what, unheld_enqueue_ms=round(1e3 * unheld_s, 3), held_enqueue_ms=round(1e3 * held_s, 3),
                    hold_asked_ms=[round(h.asked_ms, 3) for h in holds], hold_measured_ms=[round(m, 3) for m in measured]))
    assert probe.busy, '%s: hold too short (%.2f ms enqueue behind a hold of %r ms)' % (what, 1e3 * held_s, measured)
    assert min(measured) >= holds[0].asked_ms, '%s: a hold of %r ms was asked to last %.2f' % (what, measured, holds[0].asked_ms)


# ---- comparing results --------------------------------------------------------------------------------------------------------
def _bits(x):
    """Floats as integers of their width: equality of every bit, NaN and the sign of zero included."""
    import torch
    if isinstance(x, torch.Tensor):
        return x.view({4: torch.int32, 8: torch.int64, 2: torch.int16}[x.element_size()]) if x.is_floating_point() else x
    x = np.asarray(x)
    return x.view('u%d' % x.dtype.itemsize) if x.dtype.kind == 'f' else x


def same(got, want, what):
    """Two result dicts of a stage, entry by entry: torch.equal for device tensors, np.array_equal for host arrays."""
    import torch
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for key in want:
        a, b = got[key], want[key]
        if isinstance(b, torch.Tensor):
            assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(_bits(a), _bits(b)), (what, key)
        else:
            a, b = np.asarray(a), np.asarray(b)
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (what, key)


# ---- the two regimes ----------------------------------------------------------------------------------------------------------
def reference(case, data):
    """The stage on the default stream: what the existing tests pin to their oracles."""
    import torch
    out = case.drive(case.build(data), data, Probe(torch.cuda.current_stream(), []).mark)
    torch.cuda.synchronize()
    return out


def held_side_stream(case, data, other, what):
    """Regime 1 -> the results of `case` made on the default stream and driven on a fresh side stream behind a hold.  First the same
    calls run unheld on that stream on `other`, data of the same shapes: that times the enqueue the hold is sized by, and its
    released blocks are what the caching allocator hands the held run -- a misplaced launch reads stale values, not wild ones."""
    import torch
    S = torch.cuda.Stream()
    obj = case.build(other)
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        probe = Probe(S, [])
        t0 = time.perf_counter()
        out = case.drive(obj, other, probe.mark)
        unheld_s = probe.t - t0
    S.synchronize()
    del obj, out
    obj = case.build(data)
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        h = hold(S, hold_ms(unheld_s))
        probe = Probe(S, [h] if h is not None else [])
        t0 = time.perf_counter()
        out = case.drive(obj, data, probe.mark)
    S.synchronize()
    _finish(what, probe, probe.holds, t0, unheld_s)
    return out


def _construct_delayed(case, data, A, ms):
    """case.build(data) under stream A with a hold in front of every torch.zeros and torch.full of the constructor (and one in
    front of the constructor itself where it launches a kernel) -> (the stage, the holds).  ms None: no holds."""
    import torch
    holds, real = [], (torch.zeros, torch.full)

    def delayed(fn):
        def fill(*args, **kw):
            h = hold(A, ms)
            if h is not None:
                holds.append(h)
            return fn(*args, **kw)
        return fill
    if ms is not None:
        torch.zeros, torch.full = delayed(real[0]), delayed(real[1])
    try:
        with torch.cuda.stream(A):
            if ms is not None and case.init == 'kernel':
                holds.extend(h for h in [hold(A, ms)] if h is not None)
            obj = case.build(data)
    finally:
        torch.zeros, torch.full = real
    return obj, holds


def delayed_constructor(case, data, other, what):
    """Regime 2 -> the results of `case` constructed under stream A, every fill of its constructor held back, and fed under another
    stream B with nothing in between.  The unheld pass on `other` comes first, as in regime 1."""
    import torch
    A, B = torch.cuda.Stream(), torch.cuda.Stream()
    t0 = time.perf_counter()
    obj, _ = _construct_delayed(case, other, A, None)
    with torch.cuda.stream(B):
        probe = Probe(A, [])
        out = case.drive(obj, other, probe.mark)
        unheld_s = probe.t - t0
    A.synchronize()
    B.synchronize()
    del obj, out
    t0 = time.perf_counter()
    obj, holds = _construct_delayed(case, data, A, hold_ms(unheld_s))
    with torch.cuda.stream(B):
        probe = Probe(A, holds)
        out = case.drive(obj, data, probe.mark)
    A.synchronize()
    B.synchronize()
    assert holds or not HOLDS, '%s: the constructor made no fill that could be held back' % what
    _finish(what, probe, holds, t0, unheld_s)
    return out


# ---- the data -------------------------------------------------------------------------------------------------------------------
ROIS = [np.array([(y, x) for y in range(y0, y1) for x in range(x0, x1)], np.int64)
        for y0, y1, x0, x1 in ((2, 7, 3, 9), (5, 10, 7, 13), (12, 16, 20, 26), (16, 22, 30, 38), (20, 22, 2, 4))]      # 0 and 1 overlap
KEEP = np.array([t % 9 not in (3, 4) for t in range(T)])           # a run of two dropped frames in every nine
_CACHE = {}


class Recording(object):
    """T frames of a random scene cut at offsets within +-2 pixels, noise on top, the template that scene gives, and the tables
    of known shifts: numpy, and (dev()) the test's own resident copies, uploaded on the default stream and synchronised."""

    def __init__(self, dtype, seed, mode):
        rs = np.random.RandomState(100 * seed + int(np.dtype(dtype) == np.uint16))
        scene = rs.randint(0, 2000, size=(H + 8, W + 8)).astype(np.int64)
        offs = rs.randint(-2, 3, size=(T, 2))
        fr = np.stack([scene[4 + a:4 + a + H, 4 + b:4 + b + W] for a, b in offs]) + rs.randint(0, 40, size=(T, H, W))
        tmpl = scene[4:4 + H, 4:4 + W] + 20
        if np.dtype(dtype) == np.uint16:                # beyond 32767: the signedness matters
            fr, tmpl = 30 * fr, 30 * tmpl
        else:
            fr, tmpl = fr - 300, tmpl - 300             # negative values
        self.dtype, self.mode = np.dtype(dtype), mode
        self.frames, self.template = fr.astype(dtype), tmpl.astype(dtype)
        self.shifts = rs.randint(-2, 3, size=(T, 2)).astype(np.int32)
        self.fine = rs.randint(-40, 41, size=(T, 2)).astype(np.int32)
        self.weights = [rs.randint(1, 300, size=len(c)).astype(np.int64) for c in ROIS]
        self._dev = None

    def dev(self):
        import torch
        if self._dev is None:
            self._dev = (torch.from_numpy(self.frames.view(np.int16)).cuda(), torch.from_numpy(self.template.view(np.int16)).cuda())
            torch.cuda.synchronize()
        return self._dev

    @property
    def source(self):
        """What the case feeds: the resident frames, or the numpy ones (staged through the two slots)."""
        return self.dev()[0] if self.mode == 'device' else self.frames


class Matrices(object):
    """(R, TM) trace matrices: int64 sums with their areas and neuropil rows, candidate pairs, and float traces (events on noise,
    pure noise, a drifting row).  mode 'resident': the stage is given the test's own device tensors instead of numpy."""

    def __init__(self, dtype, seed, mode):
        rs = np.random.RandomState(1000 + 100 * seed + int(np.dtype(dtype) == np.float64))
        self.mode, self.dtype = mode, np.dtype(dtype)
        self.areas = rs.randint(5, 60, size=R).astype(np.int64)
        self.sums = (self.areas[:, None] * rs.randint(100, 3000, size=(R, TM))).astype(np.int64)
        self.ring_areas = np.where(np.arange(R) % 5 == 0, 0, rs.randint(20, 200, size=R)).astype(np.int64)
        self.ring_sums = (np.maximum(self.ring_areas, 1)[:, None] * rs.randint(100, 2000, size=(R, TM))).astype(np.int64)
        self.pairs = rs.randint(0, R, size=(131, 2)).astype(np.int32)
        t = np.arange(TM)
        y = np.empty((R, TM))
        for r in range(R):
            if r % 3 == 0:
                y[r] = np.convolve(rs.poisson(0.05, TM) > 0, np.exp(-t / 8.0))[:TM] + 0.2 * rs.standard_normal(TM)
            elif r % 3 == 1:
                y[r] = 0.5 * rs.standard_normal(TM)
            else:
                y[r] = 10.0 * np.cumsum(rs.standard_normal(TM)) / np.sqrt(TM) + 3.0
        self.traces = y.astype(dtype)
        self.decays = np.linspace(0.5, 0.95, R)
        self._dev = {}

    def matrix(self, name):
        """sums / ring_sums / traces as the case's mode wants them."""
        x = getattr(self, name)
        if self.mode != 'resident':
            return x
        import torch
        if name not in self._dev:
            self._dev[name] = torch.from_numpy(x).cuda()
            torch.cuda.synchronize()
        return self._dev[name]


def data_of(kind, dtype, seed, mode):
    key = (kind, np.dtype(dtype).name, seed, mode)
    if key not in _CACHE:
        _CACHE[key] = (Recording if kind == 'recording' else Matrices)(dtype, seed, mode)
    return _CACHE[key]


# ---- the stage table ----------------------------------------------------------------------------------------------------------
class Case(object):
    """One configuration of one public stage.  build(data) -> the stage, constructed on the current stream; drive(stage, data,
    mark) -> a dict of results: it feeds every chunk and takes every device result, calls mark() directly after the last launch
    that does not block the host, and only then takes what is copied to the host.
    init: how the constructor initialises device state asynchronously -- 'fills' (torch.zeros / torch.full), 'kernel', or None
    (torch.empty and uploads from numpy, which block the host until they are done): regime 2 runs the cases that have one."""

    def __init__(self, cls, name, build, drive, init=None, dtypes=DTYPES):
        self.cls, self.id, self.build, self.drive, self.init, self.dtypes = cls, '%s-%s' % (cls, name), build, drive, init, dtypes


def _feed(reader, rec, mark, then=None):
    """Feeds rec.source to `reader` (and what it returns to then()) -> the list of what feed() returned.  Resident frames go in
    one call.  Numpy frames go in a call of two chunks and mark() -- both slots are then in flight behind the hold -- and a call
    of the other four, which blocks the host once the slots wrap."""
    src = rec.source
    cuts = [(0, T)] if rec.mode == 'device' else [(0, 2 * CHUNK), (2 * CHUNK, T)]
    outs = []
    for a, b in cuts:
        out = reader.feed(src[a:b])
        outs.append(out)
        if then is not None and out.shape[0]:
            then(out)
        if len(cuts) > 1:
            mark()
    return outs


def _cat(outs):
    import torch
    return torch.cat([o for o in outs])


def _object_lists(dicts, keys):
    """A list of per-ROI dicts of exact Python ints -> one object array per key."""
    return dict((k, np.concatenate([np.atleast_1d(np.asarray(d[k], object)).ravel() for d in dicts])) for k in keys)


def _series(kinds, detrend):
    def build(rec):
        from deep_calcium_amd.series import SeriesSummarizer
        return SeriesSummarizer((H, W), T, rec.dtype, chunk_frames=CHUNK, kinds=kinds, detrend_frames=detrend)

    def drive(s, rec, mark):
        _feed(s, rec, mark)
        mark()
        out = dict((k, s.result(k)) for k in kinds)
        out['mean_standardized'] = s.result('mean', standardize=True)
        if detrend:
            m = s.result('moments')
            out['var'] = m['var']
            if m['cov'] is not None:
                out['cov'] = m['cov']
        return out
    return build, drive


def _binner():
    def build(rec):
        from deep_calcium_amd.series import SeriesSummarizer, TemporalBinner
        tb = TemporalBinner((H, W), T, rec.dtype, bin_frames=3, chunk_frames=CHUNK)
        return tb, SeriesSummarizer((H, W), tb.n_out, rec.dtype, chunk_frames=CHUNK, kinds=('mean', 'std', 'corr'))

    def drive(pair, rec, mark):
        tb, s = pair
        outs = _feed(tb, rec, mark, then=s.feed)
        binned = _cat(outs)
        mark()
        return dict(binned=binned, mean=s.result('mean'), std=s.result('std'), corr=s.result('corr'))
    return build, drive


def _quality():
    def build(rec):
        from deep_calcium_amd.frames import FrameQuality
        # the template is resident: its sums are a kernel of the constructor, on the constructor's stream
        return FrameQuality((H, W), T, rec.dtype, template=rec.dev()[1], rect=((2, H - 2), (3, W - 1)), chunk_frames=CHUNK)

    def drive(fq, rec, mark):
        _feed(fq, rec, mark)
        moments = fq.result_device('moments')
        mark()
        return dict(moments=moments, mean=fq.result_device('mean'), corr=fq.result_device('corr'))      # these read the template's sums back
    return build, drive


def _filter():
    def build(rec):
        from deep_calcium_amd.frames import FrameFilter
        return FrameFilter((H, W), T, rec.dtype, KEEP, chunk_frames=CHUNK)

    def drive(ff, rec, mark):
        kept = _cat(_feed(ff, rec, mark))
        mark()
        return dict(kept=kept)
    return build, drive


def _motion(**kw):
    def build(rec):
        from deep_calcium_amd.motion import MotionCorrector
        return MotionCorrector((H, W), T, rec.dtype, rec.template, chunk_frames=CHUNK, **kw)

    def drive(mc, rec, mark):
        out = dict(corrected=_cat(_feed(mc, rec, mark)), shifts=mc.shifts_device())
        if mc.coarse is not None:
            out['coarse'] = mc.coarse_shifts_device()
        if mc.blocks is not None:
            out['blocks'] = mc.block_shifts_device()
        if mc.subpixel:
            out['fine'] = mc.fine_shifts_device()
        mark()
        out['last_scores'] = mc.last_scores()
        return out
    return build, drive


def _bidi():
    def build(rec):
        from deep_calcium_amd.motion import BidiEstimator
        return BidiEstimator((H, W), rec.dtype, max_offset=3, chunk_frames=CHUNK)

    def drive(est, rec, mark):
        _feed(est, rec, mark)
        mark()
        return dict(scores=est.scores(), offset=np.array(est.offset()))
    return build, drive


def _known(rec, which):
    return dict(shifts=dict(shifts=rec.shifts), fine_shifts=dict(fine_shifts=rec.fine), bidi=dict(bidi=1))[which]


def _extractor(which, weighted):
    def build(rec):
        from deep_calcium_amd.traces import RoiTraceExtractor
        from deep_calcium_amd.weighted import WeightedTraceExtractor
        if weighted:
            return WeightedTraceExtractor((H, W), T, rec.dtype, ROIS, rec.weights, chunk_frames=CHUNK, **_known(rec, which))
        return RoiTraceExtractor((H, W), T, rec.dtype, ROIS, chunk_frames=CHUNK, **_known(rec, which))

    def drive(ext, rec, mark):
        _feed(ext, rec, mark)
        sums = ext.sums_device()
        mark()
        return dict(sums=sums, mean=ext.result('mean'), zscore=ext.result('zscore'))
    return build, drive


def _footprints(detrend):
    def build(rec):
        from deep_calcium_amd.footprints import RoiFootprints
        return RoiFootprints((H, W), T, rec.dtype, ROIS, halo=2, chunk_frames=CHUNK, detrend_frames=detrend)

    def drive(fp, rec, mark):
        _feed(fp, rec, mark)
        sums = fp.sums_device()
        mark()
        out = dict(sums=sums, corr=np.concatenate(fp.result('corr')), coherence=fp.result('coherence'), zscore=fp.traces('zscore'))
        out.update(_object_lists(fp.result('moments'), ('Cxx', 'Cxs', 'Css') if detrend else ('a', 'b', 'c')))
        return out
    return build, drive


def _roi_pairs(detrend):
    def build(rec):
        from deep_calcium_amd.roi_pairs import RoiPairCorr
        return RoiPairCorr((H, W), T, rec.dtype, ROIS, chunk_frames=CHUNK, detrend_frames=detrend)

    def drive(pc, rec, mark):
        _feed(pc, rec, mark)
        mark()
        out = dict(corr=np.concatenate([c.ravel() for c in pc.result('corr')]), mean=pc.traces('mean'))
        out.update(_object_lists(pc.result('moments'), ('N',) if detrend else ('a', 'g')))
        return out
    return build, drive


READERS = [
    Case('SeriesSummarizer', 'plain', *_series(('mean16', 'max16', 'mean', 'max', 'std'), None)),
    Case('SeriesSummarizer', 'corr', *_series(('mean16', 'max16', 'mean', 'max', 'std', 'corr'), None)),
    Case('SeriesSummarizer', 'detrend', *_series(('mean', 'max', 'std'), 6), init='fills'),
    Case('SeriesSummarizer', 'detrend-corr', *_series(('mean', 'max', 'std', 'corr'), 6), init='fills'),
    Case('TemporalBinner', 'then-summarizer', *_binner()),
    Case('FrameQuality', 'template', *_quality(), init='kernel'),
    Case('FrameFilter', 'keep', *_filter()),
    Case('MotionCorrector', 'rigid', *_motion(max_shift=3), init='fills'),
    Case('MotionCorrector', 'coarse', *_motion(max_shift=4, coarse=2), init='fills'),
    Case('MotionCorrector', 'blocks', *_motion(max_shift=2, blocks=(2, 2), max_dev=1), init='fills'),
    Case('MotionCorrector', 'subpixel', *_motion(max_shift=3, subpixel=True), init='fills'),
    Case('MotionCorrector', 'bidi', *_motion(max_shift=3, bidi=1, fill=7), init='fills'),
    Case('BidiEstimator', 'scores', *_bidi()),
] + [Case(cls, which, *_extractor(which, cls[0] == 'W'))
     for cls in ('RoiTraceExtractor', 'WeightedTraceExtractor') for which in ('shifts', 'fine_shifts', 'bidi')] + [
    Case('RoiFootprints', 'plain', *_footprints(None), init='fills'),
    Case('RoiFootprints', 'segments', *_footprints(6), init='fills'),
    Case('RoiPairCorr', 'plain', *_roi_pairs(None), init='fills'),
    Case('RoiPairCorr', 'segments', *_roi_pairs(6), init='fills'),
]


def _device_kinds(kinds):
    def drive(stage, m, mark):
        out = dict((k, stage.result_device(k)) for k in kinds)
        mark()
        return out
    return drive


def _baseline():
    def build(m):
        from deep_calcium_amd.dff import TraceBaseline
        return TraceBaseline(m.matrix('sums'), m.areas, 21, percentile=8, offset=3, neuropil_sums=m.matrix('ring_sums'),
                             neuropil_areas=m.ring_areas, weight=0.7)
    return build, _device_kinds(('num', 'f', 'baseline', 'dff', 'baseline_sum'))


def _trace_pairs(detrend):
    def build(m):
        from deep_calcium_amd.merge import TracePairCorr
        return TracePairCorr(m.matrix('sums'), m.areas, m.pairs, detrend_frames=detrend)
    return build, _device_kinds(('moments', 'corr'))


def _dynamics():
    def build(m):
        from deep_calcium_amd.dynamics import TraceDynamics
        return TraceDynamics(m.matrix('traces'), lags=5)
    return build, _device_kinds(('noise', 'autocov', 'g_raw'))


GAMMA, RISE = float(np.exp(-1.0 / 8)), float(np.exp(-1.0 / 2))


def _deconv(each=False, **kw):
    def build(m):
        from deep_calcium_amd.deconv import TraceDeconvolver
        return TraceDeconvolver(m.matrix('traces'), m.decays if each else GAMMA, **kw)
    searched = ('param', 'rss', 'target', 'status') if 'constrain' in kw else ()
    return build, _device_kinds(('calcium', 'spikes', 'pools', 'baseline') + searched)


FLOATS = (np.float32, np.float64)
MATRIX = [
    Case('TraceBaseline', 'neuropil', *_baseline(), dtypes=(np.int64,)),
    Case('TracePairCorr', 'plain', *_trace_pairs(None), dtypes=(np.int64,)),
    Case('TracePairCorr', 'segments', *_trace_pairs(50), dtypes=(np.int64,)),
    Case('TraceDynamics', 'lags5', *_dynamics(), dtypes=FLOATS),
    Case('TraceDeconvolver', 'plain', *_deconv(s_min=0.1, lam=0.05), dtypes=FLOATS),
    Case('TraceDeconvolver', 'each', *_deconv(each=True, s_min=0.1, lam=0.05), dtypes=FLOATS),
    Case('TraceDeconvolver', 'search-s_min', *_deconv(constrain='s_min', lam=0.02, rounds=6), dtypes=FLOATS),
    Case('TraceDeconvolver', 'search-lam', *_deconv(constrain='lam', s_min=0.1, rounds=6), dtypes=FLOATS),
    Case('TraceDeconvolver', 'fit-base', *_deconv(s_min=0.2, lam=0.01, baseline='fit', baseline_rounds=4), dtypes=FLOATS),
    Case('TraceDeconvolver', 'search-fit-base', *_deconv(constrain='s_min', baseline='fit', rounds=6), dtypes=FLOATS),
    Case('TraceDeconvolver', 'rise', *_deconv(s_min=0.1, lam=0.05, rise=RISE), dtypes=FLOATS),
    Case('TraceDeconvolver', 'rise-search', *_deconv(constrain='s_min', rise=RISE, rounds=6), dtypes=FLOATS),
]


def params(cases, modes, only=None):
    """(case, dtype, mode) for pytest.mark.parametrize, with ids -> (list, ids)."""
    out = [(c, dt, mode) for c in cases if only is None or only(c) for dt in c.dtypes for mode in modes]
    return out, ['%s-%s-%s' % (c.id, np.dtype(dt).name, mode) for c, dt, mode in out]
