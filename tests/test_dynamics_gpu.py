"""Trace dynamics on the device: dc_trace_noise, dc_trace_ar1_estimate, dc_ar1_tables and dc_trace_deconv_ar1_each against the oracles
(tests/_dyn_ref.py, tests/_deconv_ref.py), or the library's host entry point dc_trace_ar1_estimate_host where the oracle would be
slow, in every bit -- ragged tiles, padded rows, both input types, outputs pre-filled with NaN, more traces than workgroups -- and
TraceDynamics, TraceDeconvolver with a decay per trace, deconvolve_traces_device(tau='auto' | 'each') and the example on top."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _deconv_ref as dref      # noqa: E402
import _dyn_ref as ref          # noqa: E402
import _pair_ref as pair_ref    # noqa: E402

SHAPES = ((1, 1), (3, 2), (5, 3), (65, 7), (2, 255), (3, 256), (3, 257), (4, 769), (130, 1000))
LAGS = (1, 5, 16)


@pytest.fixture(scope='module')
def L(dclib):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return dclib


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _padded(y, pad):
    R, T = y.shape
    buf = np.full((R, T + pad), np.nan, y.dtype)
    buf[:, :T] = y
    return buf, torch.from_numpy(buf).cuda()


def _device_estimate(L, y, lags, pad=0, sn=None, want_sigma=True):
    """dc_trace_ar1_estimate on the rows of y, stored with stride T + pad.  The padding and the outputs are pre-filled with NaN
    (g_raw with -7): an element that is not written, or padding that is read, shows.  -> sigma, xc, g_raw."""
    R, T = y.shape
    buf, d = _padded(y, pad)
    sigma = torch.full((R,), float('nan'), dtype=torch.float64, device='cuda')
    xc = torch.full((R, lags + 1), float('nan'), dtype=torch.float64, device='cuda')
    g = torch.full((R,), -7.0, dtype=torch.float64, device='cuda')
    dsn = None if sn is None else torch.from_numpy(np.broadcast_to(np.asarray(sn, np.float64), (R,)).copy()).cuda()
    L.dc_trace_ar1_estimate(d.data_ptr(), int(y.dtype == np.float64), T + pad, R, T, lags, None if dsn is None else dsn.data_ptr(),
                            sigma.data_ptr() if want_sigma else None, xc.data_ptr(), g.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert d.cpu().numpy().tobytes() == buf.tobytes()                      # read in place, never written
    return sigma.cpu().numpy(), xc.cpu().numpy(), g.cpu().numpy()


def _device_noise(L, y, pad=0):
    R, T = y.shape
    _, d = _padded(y, pad)
    sigma = torch.full((R,), float('nan'), dtype=torch.float64, device='cuda')
    L.dc_trace_noise(d.data_ptr(), int(y.dtype == np.float64), T + pad, R, T, sigma.data_ptr(), _stream())
    torch.cuda.synchronize()
    return sigma.cpu().numpy()


def _same(got, want, what):
    for name, a, b in zip(('sigma', 'xc', 'g_raw'), got, want):
        assert ref.same_bits(a, b), (name, what, np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))[:5].tolist())


@pytest.fixture(scope='module')
def oracle():
    """The oracle's results per (R, T, lags, dtype), computed once and shared."""
    cache = {}

    def get(R, T, lags, dtype):
        key = (R, T, lags, np.dtype(dtype).name)
        if key not in cache:
            y = ref.traces(R, T, 1000 * R + T, dtype)
            cache[key] = (y, ref.estimate(y, lags))
        return cache[key]
    return get


@pytest.mark.parametrize('lags', LAGS)
@pytest.mark.parametrize('R,T', SHAPES)
def test_device_equals_the_oracle_bit_for_bit(L, oracle, R, T, lags):
    """One frame, fewer frames than lags, ragged and whole tiles of 256 frames, halo reads across a tile edge, more than one
    workgroup; padded rows (ld = T + 3, NaN), float32 and float64 traces."""
    for dtype in (np.float32, np.float64):
        y, want = oracle(R, T, lags, dtype)
        _same(_device_estimate(L, y, lags, pad=3), want, (R, T, lags, np.dtype(dtype).name))
        assert np.isnan(want[2]).all() if T < lags + 2 else not np.isnan(want[2][:3]).any()
    if (R, T) == (130, 1000):
        assert ref.same_bits(_device_noise(L, y, pad=3), want[0])


def test_device_equals_the_host_entry_on_longer_traces_and_repeats(L):
    """Seventeen frame tiles, seventy workgroups: against dc_trace_ar1_estimate_host (itself equal to the oracle in
    tests/test_dynamics_api.py); a second run gives the same bits; the caller's own noise; no sigma asked for."""
    R, T = 70, 4099
    y = ref.traces(R, T, 77, np.float32)
    for lags in (5, 16):
        want = ref.host_entry(L, y, lags)
        got = _device_estimate(L, y, lags, pad=3)
        _same(got, want, lags)
        _same(_device_estimate(L, y, lags, pad=3), got, 'second run')
    sn = np.linspace(0.0, 0.7, R)
    want = ref.host_entry(L, y, 5, sn=sn)
    _same(_device_estimate(L, y, 5, sn=sn), want, 'sn')
    got = _device_estimate(L, y, 5, sn=sn, want_sigma=False)
    assert np.isnan(got[0]).all() and ref.same_bits(got[1], want[1]) and ref.same_bits(got[2], want[2])


def test_more_traces_than_workgroups(L):
    """R past DC_TRACE_DYN_MAX_GROUPS at T = 7: every workgroup walks two or three traces."""
    from deep_calcium_amd.dynamics import MAX_GROUPS
    R, T = 2 * MAX_GROUPS + 5, 7
    y = ref.traces(R, T, 3, np.float32)
    want = ref.host_entry(L, y, 5)
    _same(_device_estimate(L, y, 5, pad=3), want, 'estimate')
    assert ref.same_bits(_device_noise(L, y, pad=3), want[0])
    rows = [0, 1, 5, MAX_GROUPS - 1, MAX_GROUPS, MAX_GROUPS + 3, 2 * MAX_GROUPS, R - 1]
    _same([a[rows] for a in want], ref.estimate(y[rows], 5), 'oracle rows')


def test_noise_equals_trace_noise_bit_for_bit(L):
    """Quantised traces -- eight levels, two levels, all equal: the selection meets ties hundreds wide -- and Gaussian ones of
    very different scale; both parities of T - 1; T < 3."""
    from deep_calcium_amd.deconv import trace_noise
    rs = np.random.RandomState(8)
    for T in (1, 2, 3, 4, 100, 101, 1000, 1001, 4097):
        quant = np.concatenate([rs.randint(0, 8, (4, T)) / 4.0, (rs.rand(2, T) < 0.5) * 1.0, np.full((1, T), 1.5), np.where(rs.rand(1, T) < 0.5, -0.0, 0.0)])
        gauss = rs.standard_normal((6, T)) * np.array([[1e-6], [0.1], [1.0], [50.0], [1e6], [1.0]]) + np.array([[0], [0], [-3], [7], [0], [1e4]])
        for y in (quant.astype(np.float32), quant, gauss.astype(np.float32), gauss):
            got = _device_noise(L, y, pad=3)
            assert ref.same_bits(got, trace_noise(y)), (T, y.dtype)
            assert not np.signbit(got).any()


@pytest.mark.parametrize('T', (1, 64, 1000))
def test_tables_equal_ar1_table_per_row(L, T):
    from deep_calcium_amd.deconv import ar1_table
    rs = np.random.RandomState(T)
    for R in (1, 63, 130):
        g = np.concatenate([[math.exp(-1.0 / 8)], rs.uniform(0.05, 0.998, R - 1)])
        G = torch.full((R, T + 4), float('nan'), dtype=torch.float64, device='cuda')
        dg = torch.from_numpy(g).cuda()
        L.dc_ar1_tables(dg.data_ptr(), R, T, G.data_ptr(), T + 4, _stream())
        torch.cuda.synchronize()
        got = G.cpu().numpy()
        assert np.isnan(got[:, T + 1:]).all()                                # entries beyond T are not written
        for r in range(R):
            assert ref.same_bits(got[r, :T + 1], ar1_table(g[r], T)), (R, T, r)


def _device_deconv_each(L, y, g, lam, smin, pad=0):
    from deep_calcium_amd.deconv import ar1_table
    R, T = y.shape
    _, d = _padded(y, pad)
    dg = torch.from_numpy(np.ascontiguousarray(g, dtype=np.float64)).cuda()
    G = torch.full((R, T + 4), float('nan'), dtype=torch.float64, device='cuda')
    L.dc_ar1_tables(dg.data_ptr(), R, T, G.data_ptr(), T + 4, _stream())
    dl = torch.from_numpy(np.broadcast_to(np.asarray(lam, np.float64), (R,)).copy()).cuda()
    ds = torch.from_numpy(np.broadcast_to(np.asarray(smin, np.float64), (R,)).copy()).cuda()
    ws = torch.full((L.dc_trace_deconv_ws_bytes(R, T) // 8,), float('nan'), dtype=torch.float64, device='cuda')
    c = torch.full((R, T), float('nan'), dtype=torch.float64, device='cuda')
    s = torch.full((R, T), float('nan'), dtype=torch.float64, device='cuda')
    n = torch.full((R,), -1, dtype=torch.int32, device='cuda')
    L.dc_trace_deconv_ar1_each(d.data_ptr(), int(y.dtype == np.float64), T + pad, R, T, dg.data_ptr(), G.data_ptr(), T + 4, dl.data_ptr(),
                               ds.data_ptr(), ws.data_ptr(), c.data_ptr(), s.data_ptr(), n.data_ptr(), _stream())
    torch.cuda.synchronize()
    out = c.cpu().numpy(), s.cpu().numpy(), n.cpu().numpy()
    # the shared entry point on the same traces, for the case of equal decays
    if np.all(np.asarray(g) == g[0]):
        G1 = torch.from_numpy(ar1_table(float(g[0]), T)).cuda()
        c1, s1, n1 = torch.empty_like(c), torch.empty_like(s), torch.empty_like(n)
        L.dc_trace_deconv_ar1(d.data_ptr(), int(y.dtype == np.float64), T + pad, R, T, float(g[0]), G1.data_ptr(), dl.data_ptr(), ds.data_ptr(),
                              ws.data_ptr(), c1.data_ptr(), s1.data_ptr(), n1.data_ptr(), _stream())
        torch.cuda.synchronize()
        return out, (c1.cpu().numpy(), s1.cpu().numpy(), n1.cpu().numpy())
    return out, None


def test_deconv_each_gives_every_trace_the_bits_of_its_own_decay(L):
    """R = 67 (a ragged second workgroup), T = 300: five distinct decays cycled over the traces, penalties that differ from row to
    row; every row against the oracle run on that row alone with its own g.  With all decays equal: the bits of dc_trace_deconv_ar1."""
    R, T = 67, 300
    rs = np.random.RandomState(4)
    t = np.arange(T)
    y = np.stack([np.convolve(rs.poisson(0.05, T) > 0, np.exp(-t / (2.0 + r % 9)))[:T] + 0.2 * rs.standard_normal(T) for r in range(R)])
    y[5] = t + 1.0                                                            # the ramp: the deepest stack
    y[6] = -1.0 * t                                                           # the collapse: one pool
    gs = np.array([math.exp(-1.0 / 2), math.exp(-1.0 / 8), math.exp(-1.0 / 30), 0.05, 0.998])[np.arange(R) % 5]
    lam = np.where(rs.rand(R) < 0.5, 0.0, 0.2 * rs.rand(R))
    smin = np.where(rs.rand(R) < 0.4, 0.0, 0.6 * rs.rand(R))
    for dtype in (np.float32, np.float64):
        yy = y.astype(dtype)
        got, _ = _device_deconv_each(L, yy, gs, lam, smin, pad=3)
        assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any() and (got[2] >= 1).all()
        for r in range(R):
            want = dref.deconvolve(yy[r:r + 1], gs[r], lam[r:r + 1], smin[r:r + 1])
            assert all(dref.same_bits(a[r:r + 1], b) for a, b in zip(got, want)), (dtype.__name__, r)
        same, shared = _device_deconv_each(L, yy, np.full(R, gs[1]), lam, smin, pad=3)
        assert all(dref.same_bits(a, b) for a, b in zip(same, shared))
        assert all(dref.same_bits(a, b) for a, b in zip(shared, dref.deconvolve(yy, gs[1], lam, smin)))


def test_trace_dynamics_numpy_and_resident_input(L):
    from deep_calcium_amd import TraceDynamics, estimate_ar1_device, pick_gamma
    R, T = 9, 700
    for dtype in (np.float32, np.float64):
        y = ref.traces(R, T, 21, dtype)
        want = ref.estimate(y, 5)
        dyn = TraceDynamics(y)
        assert dyn.result('autocov').shape == (R, 6) and dyn.result('g_raw').dtype == np.float64
        _same([dyn.result(k) for k in ('noise', 'autocov', 'g_raw')], want, dtype.__name__)
        assert dyn.result_device('g_raw') is dyn.result_device('g_raw') and dyn.result_device('noise').is_cuda       # run once
        buf, d = _padded(y, 3)
        view = d[:, :T]
        dyn = TraceDynamics(view, lags=5)
        assert dyn.traces_device.data_ptr() == d.data_ptr()                    # read in place
        _same([dyn.result(k) for k in ('noise', 'autocov', 'g_raw')], want, 'resident ' + dtype.__name__)
        assert d.cpu().numpy().tobytes() == buf.tobytes()
    sn = np.linspace(0.1, 0.5, R)
    dyn = TraceDynamics(y, lags=16, sn=sn)
    _same([dyn.result(k) for k in ('noise', 'autocov', 'g_raw')], ref.estimate(y, 16, sn=sn), 'sn')
    out = estimate_ar1_device(y, lags=5)
    g_each, status, g_pool = pick_gamma(want[2])
    assert ref.same_bits(out['g_raw'], want[2]) and ref.same_bits(out['g_each'], g_each) and out['g_pool'] == g_pool
    assert np.array_equal(out['status'], status) and ref.same_bits(out['sigma'], want[0]) and ref.same_bits(out['autocov'], want[1])
    with pytest.raises(ValueError, match='not one of'):
        dyn.result('tau')
    with pytest.raises(ValueError, match='rows of a device tensor must be contiguous'):
        TraceDynamics(torch.zeros((8, 4), device='cuda').t())


def test_trace_deconvolver_scalar_as_before_and_one_decay_per_trace(L):
    """A scalar g: the launches and the bits of dc_trace_deconv_ar1 (no table per trace is built).  An array: every row as the
    oracle gives it with that row's g."""
    from deep_calcium_amd import TraceDeconvolver
    R, T = 11, 200
    y = ref.traces(R, T, 6, np.float32)
    g = math.exp(-1.0 / 8)
    smin = np.linspace(0.0, 0.5, R)
    dec = TraceDeconvolver(y, g, s_min=smin, lam=0.05)
    dec.L.record_begin()                                                       # the launches of this thread, by name
    try:
        got = [dec.result(k) for k in ('calcium', 'spikes', 'pools')]
    finally:
        calls = [name for name, _ in dec.L.record_end()]
    assert calls == ['dc_trace_deconv_ar1']
    assert all(dref.same_bits(a, b) for a, b in zip(got, dref.deconvolve(y, g, 0.05, smin)))
    gs = np.array([0.5, g, 0.95])[np.arange(R) % 3]
    dec = TraceDeconvolver(y, gs, s_min=smin, lam=0.05)
    dec.L.record_begin()
    try:
        got = [dec.result(k) for k in ('calcium', 'spikes', 'pools')]
    finally:
        calls = [name for name, _ in dec.L.record_end()]
    assert calls == ['dc_ar1_tables', 'dc_trace_deconv_ar1_each']
    for r in range(R):
        want = dref.deconvolve(y[r:r + 1], gs[r], 0.05, smin[r:r + 1])
        assert all(dref.same_bits(a[r:r + 1], b) for a, b in zip(got, want)), r


def test_deconvolve_traces_device_auto_and_each_end_to_end(L, tmp_path):
    """A small recording (_pair_ref.scene 'two'): dF/F by dff_traces_device, then the oracles -- the estimate, pick_gamma, the
    deconvolution -- against the one call."""
    from deep_calcium_amd import deconvolve_traces_device, dff_traces_device, pick_gamma
    frames, _, left, right, _ = pair_ref.scene('two', 2)
    path = str(tmp_path / 'two.npz')
    np.savez(path, series_raw=frames)
    rois = [left, right]
    window, k = 101, 2.0
    dff = dff_traces_device(path, rois, window, percentile=20)
    sigma, _, g_raw = ref.estimate(dff, 5)
    g_each, status, g_pool = pick_gamma(g_raw)
    assert np.isfinite(g_raw).all()
    for mode, g in (('auto', np.full(2, g_pool)), ('each', g_each)):
        c, s, info = deconvolve_traces_device(path, rois, window=window, tau=mode, k=k, lam=0.05, percentile=20, details=True)
        for r in range(2):
            want = dref.deconvolve(dff[r:r + 1], g[r], 0.05, k * sigma[r:r + 1])
            assert dref.same_bits(c[r:r + 1], want[0]) and dref.same_bits(s[r:r + 1], want[1]), (mode, r)
        assert sorted(info) == ['g', 'g_raw', 'pooled', 'sigma', 'status']
        assert ref.same_bits(info['g_raw'], g_raw) and ref.same_bits(info['sigma'], sigma) and np.array_equal(info['status'], status)
        assert info['pooled'] == g_pool and (info['g'] == g_pool if mode == 'auto' else ref.same_bits(info['g'], g_each))
        two = deconvolve_traces_device(path, rois, window=window, tau=mode, fps=16.0, k=k, lam=0.05, percentile=20)
        assert len(two) == 2 and dref.same_bits(two[0], c) and dref.same_bits(two[1], s)
    # a number: today's results, and details beside them
    c0, s0 = deconvolve_traces_device(path, rois, window=window, tau=0.5, fps=16.0, k=k, percentile=20)
    c1, s1, info = deconvolve_traces_device(path, rois, window=window, tau=0.5, fps=16.0, k=k, percentile=20, details=True)
    from deep_calcium_amd import ar1_gamma
    want = dref.deconvolve(dff, ar1_gamma(0.5, 16.0), 0.0, k * sigma)
    assert dref.same_bits(c0, want[0]) and dref.same_bits(s0, want[1]) and dref.same_bits(c1, c0) and dref.same_bits(s1, s0)
    assert info['g'] == ar1_gamma(0.5, 16.0) and info['g_raw'] is None and info['pooled'] is None and ref.same_bits(info['sigma'], sigma)


def test_example_traces_command_with_deconvolve_each(L, tmp_path, monkeypatch):
    """examples/neurons/unet2ds_nf.py `traces --dff W --deconvolve each|auto --spike-k K`: `calcium` and `deconvolved` beside
    `traces`, equal to dff_traces_device followed by the oracles; the prediction is stood in for by the planted mask."""
    import importlib.util
    import os
    from deep_calcium_amd import UNet2DSummary, dff_traces_device, hdf5_min, pick_gamma
    frames, _, left, right, _ = pair_ref.scene('two', 2)
    mask2d = np.zeros(frames.shape[1:], np.float32)
    mask2d[left[:, 0], left[:, 1]] = 0.9
    mask2d[right[:, 0], right[:, 1]] = 0.9
    mask2d[:, right[:, 1].min()] = 0                          # a blank column between the two cells: two regions
    path = str(tmp_path / 'rec.npz')
    np.savez(path, series_raw=frames, series_mean=frames.mean(0).astype(np.float16), name=np.array('two'))
    script = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'examples', 'neurons', 'unet2ds_nf.py')
    state = np.random.get_state()                             # the example seeds numpy's global stream on import
    try:
        spec = importlib.util.spec_from_file_location('example_unet2ds_nf_dynamics', script)
        example = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(example)
    finally:
        np.random.set_state(state)
    monkeypatch.setattr(UNet2DSummary, 'predict', lambda self, dspaths, **kw: ([mask2d], ['two']))
    dff = dff_traces_device(path, mask2d.round().astype(np.uint8), 101, percentile=20)
    sigma, _, g_raw = ref.estimate(dff, 5)
    g_each, _, g_pool = pick_gamma(g_raw)
    for mode, g, fps in (('each', g_each, None), ('auto', np.full(2, g_pool), 16.0)):
        cp = str(tmp_path / ('cp_' + mode))
        example.traces([path], None, cp, dff=101, percentile=20, deconvolve=mode, fps=fps, spike_k=2.0)
        with hdf5_min.File(os.path.join(cp, 'two_traces.hdf5')) as f:
            assert f['traces'].read().tobytes() == dff.tobytes()
            c, s = f['calcium'].read(), f['deconvolved'].read()
        for r in range(2):
            want = dref.deconvolve(dff[r:r + 1], g[r], 0.0, 2.0 * sigma[r:r + 1])
            assert dref.same_bits(c[r:r + 1], want[0]) and dref.same_bits(s[r:r + 1], want[1]), (mode, r)
    for kw, what in ((dict(deconvolve='each'), 'needs --dff'), (dict(dff=101, deconvolve='fast'), 'auto, each or'),
                     (dict(dff=101, deconvolve='auto', fps=0.0), 'tau and fps'), (dict(dff=101, deconvolve='each', spike_k=-1.0), 'K >= 0')):
        with pytest.raises(ValueError, match=what):
            example.traces([path], None, str(tmp_path / 'cp_err'), **kw)
