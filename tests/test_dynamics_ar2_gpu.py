"""The AR(2) coefficients on the device: dc_trace_ar2_solve against the plain-Python oracle (tests/_dyn_ar2_ref.py) and against the
library's host entry point dc_trace_ar2_solve_host in every bit -- xc and sigma as the device's own dc_trace_ar1_estimate writes
them, the structural inputs, more traces than the capped grid holds, a stream that is not the default one, outputs pre-filled
with a finite sentinel (NaN is a legal result) -- and TraceDynamicsAR2, estimate_ar2_device,
deconvolve_traces_device(tau='auto', tau_rise='auto') and the example on top."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _deconv_ar2_ref as a2    # noqa: E402
import _dyn_ar2_ref as ar2      # noqa: E402
import _dyn_ref as ref          # noqa: E402

COUNTS = (1, 63, 65, 130)
LENGTHS = (3, 12, 257, 1000)
LAGS = (2, 5, 10, 16)


@pytest.fixture(scope='module')
def L(dclib):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return dclib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _device_estimate(L, y, lags):
    """dc_trace_ar1_estimate on y -> sigma [R], xc (R, lags + 1): tensors on the device, as the solve is to read them."""
    R, T = y.shape
    d = torch.from_numpy(np.ascontiguousarray(y)).cuda()
    sigma = torch.full((R,), float('nan'), dtype=torch.float64, device='cuda')
    xc = torch.full((R, lags + 1), float('nan'), dtype=torch.float64, device='cuda')
    g = torch.full((R,), -7.0, dtype=torch.float64, device='cuda')
    L.dc_trace_ar1_estimate(d.data_ptr(), int(y.dtype == np.float64), T, R, T, lags, None, sigma.data_ptr(), xc.data_ptr(), g.data_ptr(), _stream())
    torch.cuda.synchronize()
    return sigma, xc


def _device_solve(L, xc, T, lags, sn, stream=None):
    """dc_trace_ar2_solve on device tensors; the output pre-filled with a finite sentinel, the inputs checked to be unchanged.
    -> g12_raw (R, 2), numpy."""
    R = xc.shape[0]
    assert tuple(xc.shape) == (R, lags + 1) and tuple(sn.shape) == (R,) and xc.is_contiguous() and sn.is_contiguous()
    before = xc.cpu().numpy().tobytes(), sn.cpu().numpy().tobytes()
    g12 = torch.full((R, 2), ar2.SENTINEL, dtype=torch.float64, device='cuda')
    torch.cuda.synchronize()
    L.dc_trace_ar2_solve(xc.data_ptr(), R, T, lags, sn.data_ptr(), g12.data_ptr(), _stream() if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    assert (xc.cpu().numpy().tobytes(), sn.cpu().numpy().tobytes()) == before                # read, never written
    return g12.cpu().numpy()


def _check(L, xc, T, lags, sn, what, stream=None):
    """The device against the oracle and against the host entry point, on the same xc and sn."""
    got = _device_solve(L, xc, T, lags, sn, stream)
    xh, sh = xc.cpu().numpy(), sn.cpu().numpy()
    want = ar2.solve_rows(xh, T, lags, sh)
    assert ref.same_bits(got, want), (what, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5].tolist())
    assert ref.same_bits(ar2.host_entry(L, xh, T, lags, sh), want), what
    assert not (got == ar2.SENTINEL).any()
    return got


@pytest.fixture(scope='module')
def traces():
    cache = {}

    def get(R, T):
        if (R, T) not in cache:
            cache[(R, T)] = ref.traces(R, T, 1000 * R + T, np.float32)
        return cache[(R, T)]
    return get


@pytest.mark.parametrize('lags', LAGS)
@pytest.mark.parametrize('R', COUNTS)
def test_device_equals_the_oracle_bit_for_bit(L, traces, R, lags):
    """One trace, a ragged and a whole workgroup of 64 lanes, more than two; fewer frames than lags + 2 (undefined: NaN), and
    enough; xc and sigma from the device's own estimate of the same traces."""
    for T in LENGTHS:
        sigma, xc = _device_estimate(L, traces(R, T), lags)
        got = _check(L, xc, T, lags, sigma, (R, T, lags))
        assert np.isnan(got).all() if T < lags + 2 else (np.isnan(got[:, 0]) == np.isnan(got[:, 1])).all()
        if T == 1000:
            assert np.isfinite(got[0]).all()                                                # events on noise: defined


def test_device_equals_the_whole_oracle_and_the_callers_noise(L, traces):
    """Against the oracle from the traces on (its own folds, its own noise), not only from the device's xc; and with sn given."""
    R, T = 65, 257
    y = traces(R, T)
    for lags in LAGS:
        sigma, xc = _device_estimate(L, y, lags)
        s, x, _, want = ar2.estimate(y, lags)
        assert ref.same_bits(sigma.cpu().numpy(), s) and ref.same_bits(xc.cpu().numpy(), x)
        assert ref.same_bits(_device_solve(L, xc, T, lags, sigma), want), lags
        sn = np.linspace(0.0, 0.7, R)
        want = ar2.estimate(y, lags, sn=sn)[3]
        assert ref.same_bits(_device_solve(L, xc, T, lags, torch.from_numpy(sn).cuda()), want), (lags, 'sn')


def test_structural_inputs(L):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()               # noqa: E731
    for lags in LAGS:
        zero = dev(np.zeros((3, lags + 1)))
        assert np.isnan(_check(L, zero, 1000, lags, dev(np.zeros(3)), 'zero')).all()            # det == 0.0
        assert (_check(L, zero, 1000, lags, dev(np.full(3, 0.5)), 'zero, sn') == 0.0).all()     # sn alone fills the diagonal
        y = np.full((2, 300), 1.5, np.float32)                                                  # a constant trace: no covariance
        sigma, xc = _device_estimate(L, y, lags)
        assert xc.cpu().numpy().tobytes() == np.zeros((2, lags + 1)).tobytes()
        assert np.isnan(_check(L, xc, 300, lags, sigma, 'constant')).all()
        y = ref.traces(6, 400, 5, np.float64)                                                   # sn so large that c0 < 0
        _, xc = _device_estimate(L, y, lags)
        sn = 2.0 * torch.sqrt(xc[:, 0]) + 1.0
        assert bool(((xc[:, 0] - sn * sn) < 0).all())
        _check(L, xc, 400, lags, sn.contiguous(), 'c0 < 0')
        y = ref.traces(2, lags + 2, 12, np.float64)                                             # T = lags + 1 against lags + 2
        s1, x1 = _device_estimate(L, np.ascontiguousarray(y[:, :lags + 1]), lags)
        s2, x2 = _device_estimate(L, y, lags)
        assert np.isnan(_check(L, x1, lags + 1, lags, s1, 'T = lags + 1')).all()
        assert not np.isnan(_check(L, x2, lags + 2, lags, s2, 'T = lags + 2')).any()
        assert np.isnan(_check(L, x2, lags + 1, lags, s2, 'T alone decides')).all()
        assert np.isnan(_check(L, x2, 0, lags, s2, 'T = 0')).all()
    # R == 0: nothing is launched, nothing is written
    g12 = torch.full((2, 2), ar2.SENTINEL, dtype=torch.float64, device='cuda')
    assert L.dc_trace_ar2_solve(x2.data_ptr(), 0, 1000, 16, s2.data_ptr(), g12.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert bool((g12 == ar2.SENTINEL).all())


def test_more_traces_than_the_grid_holds(L):
    """R = 2 * DC_TRACE_DYN_MAX_GROUPS * 64 + 5 at lags = 2: the grid is capped at DC_TRACE_DYN_MAX_GROUPS workgroups of 64 lanes, so
    every lane walks two traces and five walk three.  xc: the device's estimate of 130 traces, repeated, every copy scaled by its
    own factor and with its own noise, so that no two rows give the same result.  Against the host entry point everywhere (equal
    to the oracle by the tests above) and the oracle on rows of every trip."""
    from deep_calcium_amd.dynamics import MAX_GROUPS
    R, lags, T = 2 * MAX_GROUPS * 64 + 5, 2, 257
    sigma, xc = _device_estimate(L, ref.traces(130, T, 9, np.float32), lags)
    rs = np.random.RandomState(2)
    reps = (R + 129) // 130
    scale = torch.from_numpy(rs.uniform(0.5, 2.0, R)).cuda()
    big = (xc.repeat(reps, 1)[:R] * scale[:, None]).contiguous()
    sn = (sigma.repeat(reps)[:R] * torch.from_numpy(rs.uniform(0.0, 1.5, R)).cuda()).contiguous()
    got = _device_solve(L, big, T, lags, sn)
    xh, sh = big.cpu().numpy(), sn.cpu().numpy()
    want = ar2.host_entry(L, xh, T, lags, sh)
    assert ref.same_bits(got, want), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5].tolist()
    lanes = MAX_GROUPS * 64
    rows = [0, 1, 63, 64, lanes - 1, lanes, lanes + 1, 2 * lanes - 1, 2 * lanes, 2 * lanes + 4]
    assert rows[-1] == R - 1
    assert ref.same_bits(got[rows], ar2.solve_rows(xh[rows], T, lags, sh[rows]))
    assert np.isfinite(got).any() and len(np.unique(got[np.isfinite(got[:, 0]), 0])) > R // 4


def test_on_a_stream_that_is_not_the_default(L, traces):
    R, T, lags = 130, 1000, 10
    sigma, xc = _device_estimate(L, traces(R, T), lags)
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.default_stream().cuda_stream
    got = _check(L, xc, T, lags, sigma, 'side stream', stream=side)
    assert ref.same_bits(got, _device_solve(L, xc, T, lags, sigma))


def _stage_case():
    """TraceDynamicsAR2 as a case of the stream tests (tests/_streams.py: its matrices, its hold, its probe)."""
    import _streams as st

    def build(m):
        from deep_calcium_amd import TraceDynamicsAR2
        return TraceDynamicsAR2(m.matrix('traces'), lags=10)

    def drive(stage, m, mark):
        out = dict((k, stage.result_device(k)) for k in ('noise', 'autocov', 'g_raw', 'g12_raw'))
        mark()
        return out
    return st, st.Case('TraceDynamics', 'ar2-lags10', build, drive, dtypes=st.FLOATS)


@pytest.mark.parametrize('mode', ('numpy', 'resident'))
@pytest.mark.parametrize('dtype', (np.float32, np.float64))
def test_stage_on_a_held_side_stream(L, dtype, mode):
    """The stage of order 2 as tests/test_streams_gpu.py runs every stage of its table: constructed on the default stream, both
    launches enqueued on a fresh side stream behind a hold that is proved to have held -- the bits of the default-stream run.  A
    solve that lost its stream argument would read an xc that the held estimate has not written yet."""
    st, case = _stage_case()
    st._units_per_ms(torch)                                                    # the hold's calibration, outside every timed region
    torch.cuda.synchronize()
    want = st.reference(case, st.data_of('matrix', dtype, 0, 'numpy'))
    assert torch.isfinite(want['g12_raw']).any()
    what = 'held %s-%s-%s' % (case.id, np.dtype(dtype).name, mode)
    got = st.held_side_stream(case, st.data_of('matrix', dtype, 0, mode), st.data_of('matrix', dtype, 1, mode), what)
    st.same(got, want, what)


def test_trace_dynamics_ar2_numpy_and_resident_input(L):
    from deep_calcium_amd import TraceDynamics, TraceDynamicsAR2, estimate_ar2_device, pick_roots
    from deep_calcium_amd.dynamics import AR2_KINDS
    R, T = 9, 700
    for dtype in (np.float32, np.float64):
        y = ref.traces(R, T, 21, dtype)
        want = ar2.estimate(y, 10)
        dyn = TraceDynamicsAR2(y)
        assert isinstance(dyn, TraceDynamics) and dyn.order == 2 and dyn.kinds == AR2_KINDS and dyn.lags == 10
        dyn.L.record_begin()                                                   # the launches of this thread, by name
        try:
            g12 = dyn.result()
        finally:
            calls = [name for name, _ in dyn.L.record_end()]
        assert calls == ['dc_trace_ar1_estimate', 'dc_trace_ar2_solve']
        assert g12.shape == (R, 2) and g12.dtype == np.float64 and dyn.result('autocov').shape == (R, 11)
        for kind, b in zip(('noise', 'autocov', 'g_raw', 'g12_raw'), want):
            assert ref.same_bits(dyn.result(kind), b), (kind, dtype.__name__)
        assert dyn.result_device('g12_raw') is dyn.result_device('g12_raw') and dyn.result_device().is_cuda        # run once
        buf = np.full((R, T + 3), np.nan, dtype)
        buf[:, :T] = y
        d = torch.from_numpy(buf).cuda()
        dyn = TraceDynamicsAR2(d[:, :T], lags=10)
        assert dyn.traces_device.data_ptr() == d.data_ptr()                    # read in place
        for kind, b in zip(('noise', 'autocov', 'g_raw', 'g12_raw'), want):
            assert ref.same_bits(dyn.result(kind), b), ('resident', kind, dtype.__name__)
        assert d.cpu().numpy().tobytes() == buf.tobytes()
    sn = np.linspace(0.1, 0.5, R)
    dyn = TraceDynamicsAR2(y, lags=16, sn=sn)
    assert ref.same_bits(dyn.result('g12_raw'), ar2.estimate(y, 16, sn=sn)[3])
    out = estimate_ar2_device(y, lags=10, fallback=(0.9, 0.5))
    roots_each, status, pooled = ar2.pick_roots(want[3], fallback=(0.9, 0.5))
    assert ref.same_bits(out['g12_raw'], want[3]) and ref.same_bits(out['roots_each'], roots_each) and out['pooled'] == pooled
    assert np.array_equal(out['status'], status) and ref.same_bits(out['sigma'], want[0]) and ref.same_bits(out['autocov'], want[1])
    assert ref.same_bits(out['g_raw'], want[2]) and out['pooled'] == pick_roots(want[3], fallback=(0.9, 0.5))[2]
    with pytest.raises(ValueError, match='not one of noise, autocov, g_raw, g12_raw'):
        dyn.result('tau')
    with pytest.raises(ValueError, match='not one of noise, autocov, g_raw$'):
        TraceDynamics(y).result('g12_raw')


def _same_deconvolution(got_c, got_s, dec):
    return ref.same_bits(got_c, dec.result('calcium')) and ref.same_bits(got_s, dec.result('spikes'))


def test_deconvolve_traces_device_with_both_roots_estimated(L, tmp_path):
    """A small recording of nine cells with a rise time, T = 700: dF/F by dff_traces_device, the oracle's estimate and its pooled
    roots, TraceDeconvolver at those roots -- against the one call, with a numeric k and with the threshold searched."""
    from deep_calcium_amd import TraceDeconvolver, deconvolve_traces_device, dff_traces_device
    frames, rois = ar2.recording(1)
    path = str(tmp_path / 'nine.npz')
    np.savez(path, series_raw=frames)
    window, k = 101, 2.0
    dff = dff_traces_device(path, rois, window, percentile=20)
    assert dff.shape == (9, 700)
    sigma, _, g_raw, g12 = ar2.estimate(dff, 10)
    _, status, (d, r) = ar2.pick_roots(g12)
    assert (status == 0).sum() >= 3 and 0.0 < r < d < 1.0
    c, s, info = deconvolve_traces_device(path, rois, window=window, tau='auto', tau_rise='auto', k=k, lam=0.05, percentile=20, details=True)
    assert _same_deconvolution(c, s, TraceDeconvolver(dff, d, rise=r, s_min=k * sigma, lam=0.05))
    want = a2.deconvolve(dff[:2], d, r, 0.05, k * sigma[:2])                   # and the oracle of the deconvolution on two of them
    assert ref.same_bits(c[:2], want[0]) and ref.same_bits(s[:2], want[1])
    assert sorted(info) == ['g', 'g12_raw', 'g_raw', 'pooled', 'rise', 'root_status', 'sigma', 'status']
    assert info['g'] == d and info['rise'] == r and info['pooled'] == (d, r) and info['status'] is None
    assert ref.same_bits(info['g12_raw'], g12) and np.array_equal(info['root_status'], status) and info['root_status'].dtype == np.int8
    assert ref.same_bits(info['sigma'], sigma) and ref.same_bits(info['g_raw'], g_raw)
    assert ((s > 0).sum(1) >= 1).all()
    two = deconvolve_traces_device(path, rois, window=window, tau='auto', tau_rise='auto', fps=16.0, k=k, lam=0.05, percentile=20)
    assert len(two) == 2 and ref.same_bits(two[0], c) and ref.same_bits(two[1], s)
    # the threshold searched: sigma stays on the device
    c, s, info = deconvolve_traces_device(path, rois, window=window, tau='auto', tau_rise='auto', k='noise', percentile=20, details=True)
    dec = TraceDeconvolver(dff, d, rise=r, constrain='s_min', sigma=sigma)
    assert _same_deconvolution(c, s, dec)
    assert ref.same_bits(info['s_min'], dec.result('param')) and ref.same_bits(info['rss'], dec.result('rss'))
    assert np.array_equal(info['search_status'], dec.result('status')) and info['pooled'] == (d, r)
    # other lags: another estimate, its own pooled roots
    c5, s5, info5 = deconvolve_traces_device(path, rois, window=window, tau='auto', tau_rise='auto', rise_lags=5, k=k, percentile=20, details=True)
    _, _, pooled5 = ar2.pick_roots(ar2.estimate(dff, 5)[3])
    assert info5['pooled'] == pooled5 != (d, r)
    assert _same_deconvolution(c5, s5, TraceDeconvolver(dff, pooled5[0], rise=pooled5[1], s_min=k * sigma))
    # tau='auto' alone is what it was: AR(1), and its info has no new key
    _, _, info1 = deconvolve_traces_device(path, rois, window=window, tau='auto', k=k, percentile=20, details=True)
    assert sorted(info1) == ['g', 'g_raw', 'pooled', 'sigma', 'status']


def test_example_traces_command_with_spike_rise_auto(L, tmp_path, monkeypatch, caplog):
    """examples/neurons/unet2ds_nf.py `traces --dff W --deconvolve auto --spike-rise auto`: `calcium` and `deconvolved` beside
    `traces`, the datasets deconvolve_traces_device gives; the prediction is stood in for by the planted mask.  The log names the
    pooled roots, the coefficients, the frame of the peak, the status counts and, with --fps, both time constants."""
    import importlib.util
    import logging
    import os
    from deep_calcium_amd import UNet2DSummary, ar1_tau, deconvolve_traces_device, dff_traces_device, hdf5_min
    from deep_calcium_amd.deconv import ar2_peak
    frames, rois = ar2.recording(1)
    mask2d = np.zeros(frames.shape[1:], np.float32)
    for roi in rois:
        mask2d[roi[:, 0], roi[:, 1]] = 0.9
    path = str(tmp_path / 'rec.npz')
    np.savez(path, series_raw=frames, series_mean=frames.mean(0).astype(np.float16), name=np.array('nine'))
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'neurons', 'unet2ds_nf.py')
    state = np.random.get_state()                             # the example seeds numpy's global stream on import
    try:
        spec = importlib.util.spec_from_file_location('example_unet2ds_nf_dynamics_ar2', script)
        example = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(example)
    finally:
        np.random.set_state(state)
    monkeypatch.setattr(UNet2DSummary, 'predict', lambda self, dspaths, **kw: ([mask2d], ['nine']))
    mask = mask2d.round().astype(np.uint8)
    dff = dff_traces_device(path, mask, 101, percentile=20)
    assert dff.shape == (9, 700)
    c, s, info = deconvolve_traces_device(path, mask, window=101, tau='auto', tau_rise='auto', k=2.0, percentile=20, details=True)
    d, r = info['pooled']
    assert (d, r) == ar2.pick_roots(ar2.estimate(dff, 10)[3])[2]
    cp = str(tmp_path / 'cp')
    with caplog.at_level(logging.INFO):
        example.traces([path], None, cp, dff=101, percentile=20, deconvolve='auto', fps=16.0, spike_k=2.0, spike_rise='auto')
    with hdf5_min.File(os.path.join(cp, 'nine_traces.hdf5')) as f:
        assert f['traces'].read().tobytes() == dff.tobytes()
        assert ref.same_bits(f['calcium'].read(), c) and ref.same_bits(f['deconvolved'].read(), s)
    g1, g2 = a2.coefficients(d, r)
    counts = np.bincount(info['root_status'], minlength=5)
    assert 'pooled d = %.6f, r = %.6f (tau %.4g s, tau_rise %.4g s at 16 frames/s), g1 = %.6f, g2 = %.6f' % (
        d, r, ar1_tau(d, 16.0), ar1_tau(r, 16.0), g1, g2) in caplog.text
    assert 'peaks at frame %d' % ar2_peak(d, r) in caplog.text and '= %d / %d / %d / %d / %d;' % tuple(counts) in caplog.text
    c, s, _ = deconvolve_traces_device(path, mask, window=101, tau='auto', tau_rise='auto', k='noise', percentile=20, details=True)
    cp = str(tmp_path / 'cp_searched')
    example.traces([path], None, cp, dff=101, percentile=20, deconvolve='auto', spike_constrain='s_min', spike_rise='auto')
    with hdf5_min.File(os.path.join(cp, 'nine_traces.hdf5')) as f:
        assert ref.same_bits(f['calcium'].read(), c) and ref.same_bits(f['deconvolved'].read(), s)
    for kw, what in ((dict(dff=101, deconvolve='auto', spike_rise=0.1), 'needs --deconvolve TAU'),
                     (dict(dff=101, deconvolve=0.5, fps=16.0, spike_rise='auto'), '--spike-rise auto estimates both roots'),
                     (dict(dff=101, deconvolve='each', spike_rise='auto'), '--spike-rise auto estimates both roots'),
                     (dict(dff=101, deconvolve='auto', spike_rise='auto', spike_baseline='fit'), 'not built for AR'),
                     (dict(dff=101, deconvolve='auto', spike_rise='fast'), 'takes auto or the rise time')):
        with pytest.raises(ValueError, match=what):
            example.traces([path], None, str(tmp_path / 'cp_err'), **kw)
