"""The AR(2) deconvolution on the device: dc_trace_deconv_ar2 against the plain-Python oracle (tests/_deconv_ar2_ref.py), or the
library's host entry point dc_trace_deconv_ar2_host where the oracle would be slow, in every bit of calcium, spikes and pools --
ragged tiles of traces and frames, the two special frames of the penalty, padded rows, both input types, per-trace penalties and
baselines, divergent lanes, buffers pre-filled with NaN --; dc_trace_deconv_ar2_constrained against
dc_trace_deconv_ar2_constrained_host; and TraceDeconvolver(rise=) / deconvolve_traces_device(tau_rise=) / the example's
--spike-rise on top of them."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _deconv_ar2_ref as a2    # noqa: E402
import _deconv_ref as ref       # noqa: E402
import _deconv_search_ref as sr # noqa: E402
import _pair_ref as pair_ref    # noqa: E402
from test_deconv_gpu import _penalties, _traces      # noqa: E402

LANES = 64                      # traces per workgroup of the forward kernel
FRAMES = 64                     # frames per staged tile
CANARY = -77.25
GUARD = 5                       # canary elements / rows behind every output of the search


@pytest.fixture(scope='module')
def L(dclib):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return dclib


def _on_device(y, d, r, pad):
    """The rows of y with stride T + pad and the table with rows of stride T + 1 + pad, the padding NaN -> what the entry points take."""
    from deep_calcium_amd.deconv import ar2_table
    buf, R, T = a2._padded(y, pad)
    H = a2._padded(ar2_table(d, r, T), pad)[0]
    g1, g2 = a2.coefficients(float(d), float(r))
    return buf, torch.from_numpy(buf).cuda(), torch.from_numpy(H).cuda(), g1, g2


def _vector(x, R):
    return torch.from_numpy(np.broadcast_to(np.asarray(x, np.float64), (R,)).copy()).cuda()


def _device_run(L, y, d, r, lam, smin, base=None, pad=0):
    """dc_trace_deconv_ar2 on the rows of y.  The padding, the outputs and the workspace are pre-filled with NaN (pools with -1): an
    element that is not written, or padding that is read, shows.  -> calcium, spikes, pools."""
    R, T = y.shape
    buf, dy, H, g1, g2 = _on_device(y, d, r, pad)
    dl, ds = _vector(lam, R), _vector(smin, R)
    db = None if base is None else _vector(base, R)
    nbytes = L.dc_trace_deconv_ar2_ws_bytes(R, T)
    assert nbytes == 40 * R * T
    ws = torch.full((nbytes // 8,), float('nan'), dtype=torch.float64, device='cuda')
    c = torch.full((R, T), float('nan'), dtype=torch.float64, device='cuda')
    s = torch.full((R, T), float('nan'), dtype=torch.float64, device='cuda')
    n = torch.full((R,), -1, dtype=torch.int32, device='cuda')
    L.dc_trace_deconv_ar2(dy.data_ptr(), int(y.dtype == np.float64), T + pad, R, T, g1, g2, H.data_ptr(), T + 1 + pad, dl.data_ptr(), ds.data_ptr(),
                          None if db is None else db.data_ptr(), ws.data_ptr(), c.data_ptr(), s.data_ptr(), n.data_ptr(),
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert dy.cpu().numpy().tobytes() == buf.tobytes()                     # read in place, never written
    return c.cpu().numpy(), s.cpu().numpy(), n.cpu().numpy()


def _same(got, want, what):
    for name, a, b in zip(('calcium', 'spikes', 'pools'), got, want):
        assert not np.isnan(a).any() if a.dtype.kind == 'f' else (a >= 1).all(), (name, what)
        assert ref.same_bits(a, b), (name, what, np.argwhere(a != b)[:5].tolist())


@pytest.mark.parametrize('T', (1, 2, 3, FRAMES - 1, FRAMES, FRAMES + 1, 257))
@pytest.mark.parametrize('R', (1, LANES - 1, LANES, LANES + 1, 130))
def test_device_equals_the_oracle_bit_for_bit(L, R, T):
    """Ragged tiles in both directions; T = 2 and 3, where sec falls back to u and the penalty has its two special frames; padded
    rows (ld = T + 3), float32 and float64, penalties that differ from row to row, a given baseline per row on half the runs, and
    the ramp, the collapse and the cascade in lanes next to ordinary traces."""
    seed = 1000 * R + T
    d, r = a2.ROOTS[(R + T) % 4]
    y64 = _traces(R, T, seed)
    lam, smin = _penalties(R, seed)
    base = 0.3 * np.random.RandomState(seed + 2).standard_normal(R)
    for dtype, pad, b in ((np.float32, 3, None), (np.float64, 0, base), (np.float64, 3, None), (np.float32, 0, base)):
        y = y64.astype(dtype)
        want = a2.deconvolve(y, d, r, lam, smin, b)
        _same(_device_run(L, y, d, r, lam, smin, b, pad=pad), want, (R, T, dtype.__name__, pad, b is not None))
        if b is None and R > 5:
            assert want[2][3] == T and want[2][4] == 1                     # the ramp kept every pool, the collapse one
            assert want[0][4].tobytes() == np.zeros(T).tobytes() and want[1][4].tobytes() == np.zeros(T).tobytes()


def test_device_equals_the_host_entry_on_longer_traces_and_repeats(L):
    """Several workgroups, sixteen frame tiles, stacks hundreds deep: against dc_trace_deconv_ar2_host (itself equal to the oracle
    in tests/test_deconv_ar2_api.py); a sample of rows against the oracle as well; and a second run gives the same bits."""
    R, T = 300, 1000
    y = _traces(R, T, 77).astype(np.float32)
    lam, smin = _penalties(R, 77)
    for d, r in (a2.ROOTS[1], a2.ROOTS[2]):
        want = a2.host_entry(L, y, d, r, lam, smin)
        got = _device_run(L, y, d, r, lam, smin, pad=3)
        _same(got, want, (d, r))
        again = _device_run(L, y, d, r, lam, smin, pad=3)
        _same(again, got, 'second run')
        rows = [0, 3, 4, 5, 64, 65, 128, 255, 256, 299]
        _same([a[rows] for a in got], a2.deconvolve(y[rows], d, r, lam[rows], smin[rows]), 'oracle rows')
        assert got[2].max() == T and got[2].min() == 1


# ---- the noise-constrained search ----------------------------------------------------------------------------------------------------
def _mixed(R, T, seed, d, r):
    """Rows in turn, so that the lanes of a wave end differently: AR(2) events on noise held to their noise, an all-zero row held
    to sigma 1 (never bracketed), a noiseless event train held to sigma 0 (status 1), pure noise held to twice its level.
    -> y float64 (R, T), sigma float64[R]."""
    rs = np.random.RandomState(seed)
    y, sigma = np.zeros((R, T)), np.zeros(R)
    kernel = np.array(a2.table(d, r, T)[0][:T])
    kernel = kernel / kernel.max()
    for i in range(R):
        kind = i % 4
        sp = rs.poisson(0.05, T) > 0
        if kind == 0:
            sigma[i] = 0.1 + 0.3 * rs.rand()
            y[i] = np.convolve(sp, kernel)[:T] + sigma[i] * rs.standard_normal(T)
        elif kind == 1:
            sigma[i] = 1.0
        elif kind == 2:
            y[i] = np.convolve(sp, kernel)[:T]
        else:
            y[i] = 0.25 * rs.standard_normal(T)
            sigma[i] = 0.5
    return y, sigma


def _device_search(L, y, d, r, which, sigma, other=0.0, rounds=6, pad=0, resident=None):
    """dc_trace_deconv_ar2_constrained on the rows of y.  The padding and the workspace are pre-filled with NaN; every output is GUARD
    elements (rows) longer than it need be and pre-filled with a canary: what is not written, or written beyond row R, shows.
    resident: a tensor that already holds the rows (ld = its stride) -- it is the one read.  -> dict like the oracle's."""
    R, T = y.shape
    buf, dy, H, g1, g2 = _on_device(y, d, r, pad)
    if resident is not None:
        dy, buf, pad = resident, resident.cpu().numpy(), resident.stride(0) - T
    dsig, doth = _vector(sigma, R), _vector(other, R)
    assert L.dc_trace_deconv_search_state_bytes(R) == 40 * R
    ws = torch.full((5 * R * T + GUARD,), float('nan'), dtype=torch.float64, device='cuda')
    ws[5 * R * T:] = CANARY
    state = torch.full((5 * R + GUARD,), CANARY, dtype=torch.float64, device='cuda')
    c = torch.full((R + GUARD, T), CANARY, dtype=torch.float64, device='cuda')
    s = torch.full((R + GUARD, T), CANARY, dtype=torch.float64, device='cuda')
    n = torch.full((R + GUARD,), -7, dtype=torch.int32, device='cuda')
    param = torch.full((R + GUARD,), CANARY, dtype=torch.float64, device='cuda')
    rss = torch.full((R + GUARD,), CANARY, dtype=torch.float64, device='cuda')
    status = torch.full((R + GUARD,), -7, dtype=torch.int32, device='cuda')
    L.dc_trace_deconv_ar2_constrained(dy.data_ptr(), int(y.dtype == np.float64), T + pad, R, T, g1, g2, H.data_ptr(), H.stride(0), which,
                                      dsig.data_ptr(), doth.data_ptr(), rounds, ws.data_ptr(), state.data_ptr(), c.data_ptr(), s.data_ptr(),
                                      n.data_ptr(), param.data_ptr(), rss.data_ptr(), status.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert dy.cpu().numpy().tobytes() == buf.tobytes()                     # read in place, never written
    for name, a in (('calcium', c), ('spikes', s), ('param', param), ('rss', rss)):
        assert (a[R:].cpu().numpy() == CANARY).all(), (name, 'written beyond row R')
    assert (n[R:].cpu().numpy() == -7).all() and (status[R:].cpu().numpy() == -7).all()
    assert (ws[5 * R * T:].cpu().numpy() == CANARY).all() and (state[5 * R:].cpu().numpy() == CANARY).all()
    return dict(param=param[:R].cpu().numpy(), rss=rss[:R].cpu().numpy(), status=status[:R].cpu().numpy(), target=state[3 * R:4 * R].cpu().numpy(),
                calcium=c[:R].cpu().numpy(), spikes=s[:R].cpu().numpy(), pools=n[:R].cpu().numpy())


@pytest.mark.parametrize('rounds', (1, 24))
@pytest.mark.parametrize('T', (2, 257))
@pytest.mark.parametrize('R', (1, 65))
def test_search_equals_the_host_entry_bit_for_bit(L, R, T, rounds):
    """dc_trace_deconv_ar2_constrained against dc_trace_deconv_ar2_constrained_host (itself equal to the oracle in
    tests/test_deconv_ar2_api.py) in calcium, spikes, pools, param, rss and status; both parameters, the other one fixed at zero and
    above it; traces held to sigma = 0 (status 1) and pure-noise traces among the lanes of a wave; a few rows against the oracle."""
    seed = 1000 * R + T + rounds
    d, r = a2.ROOTS[(R + T + rounds) % 3]
    y64, sigma = _mixed(R, T, seed, d, r)
    for dtype, pad, which, other in ((np.float32, 3, sr.SMIN, 0.0), (np.float64, 0, sr.LAM, 0.0), (np.float64, 3, sr.SMIN, 0.05),
                                     (np.float32, 0, sr.LAM, 0.1)):
        y = y64.astype(dtype)
        want = a2.host_constrained(L, y, d, r, which, sigma, other, rounds)
        got = _device_search(L, y, d, r, which, sigma, other, rounds, pad=pad)
        a2.same(got, want, (R, T, rounds, dtype.__name__, pad, which))
        assert ref.same_bits(got['target'], (sigma * sigma) * float(T))
        assert (got['status'][sigma == 0.0] == 1).all() and (got['rss'] <= got['target'])[got['status'] != 1].all()
    rows = list(range(min(R, 4)))
    a2.same({k: v[rows] for k, v in got.items()}, a2.constrained(y[rows], d, r, which, sigma[rows], other, rounds), 'oracle rows')


def test_search_with_more_traces_than_residual_workgroups_and_resident_input(L):
    """Beyond DC_TRACE_DECONV_SEARCH_MAX_GROUPS = 8192 traces a workgroup of the residual kernel walks several; and a tensor that
    already lies on the device, with padded rows, is read in place."""
    R, T, rounds = 8200, 5, 3
    d, r = a2.ROOTS[1]
    y64, sigma = _mixed(R, T, 5, d, r)
    y = y64.astype(np.float32)
    got = _device_search(L, y, d, r, sr.SMIN, sigma, 0.0, rounds, pad=1)
    want = a2.host_constrained(L, y, d, r, sr.SMIN, sigma, 0.0, rounds)
    a2.same(got, want, 'capped grid')
    rows = [0, 1, 2, 3, 8191, 8192, 8193, R - 1]
    a2.same({k: v[rows] for k, v in got.items()}, a2.constrained(y[rows], d, r, sr.SMIN, sigma[rows], 0.0, rounds), 'oracle rows')
    R, T = 70, 130
    y64, sigma = _mixed(R, T, 6, d, r)
    held = torch.full((R, T + 3), float('nan'), dtype=torch.float64, device='cuda')
    held[:, :T] = torch.from_numpy(y64).cuda()
    got = _device_search(L, y64, d, r, sr.LAM, sigma, 0.02, 7, resident=held)
    a2.same(got, a2.host_constrained(L, y64, d, r, sr.LAM, sigma, 0.02, 7), 'resident')
    assert set(got['status'].tolist()) == {0, 1, 2}


# ---- the front end -------------------------------------------------------------------------------------------------------------------
def test_trace_deconvolver_with_a_rise_time(L):
    from deep_calcium_amd import TraceDeconvolver
    from deep_calcium_amd.deconv import trace_noise
    R, T = 70, 130
    d, r = a2.ROOTS[1]
    y64 = _traces(R, T, 5)
    lam, smin = _penalties(R, 5)
    base = 0.2 * np.random.RandomState(8).standard_normal(R)
    three = ('calcium', 'spikes', 'pools')
    for dtype in (np.float32, np.float64):
        y = y64.astype(dtype)
        want = a2.deconvolve(y, d, r, lam, smin)
        dec = TraceDeconvolver(y, d, s_min=smin, lam=lam, rise=r)
        assert dec.result('calcium').dtype == np.float64 and dec.result('pools').dtype == np.int32
        _same([dec.result(k) for k in three], want, dtype.__name__)
        assert dec.result_device('spikes') is dec.result_device('spikes') and dec.result_device('calcium').is_cuda      # run once
        assert dec.result('baseline').tobytes() == np.zeros(R).tobytes()
        # a resident tensor with padded rows: read in place and left unchanged; a given baseline per trace
        buf = np.full((R, T + 3), np.nan, dtype)
        buf[:, :T] = y
        held = torch.from_numpy(buf).cuda()
        dec = TraceDeconvolver(held[:, :T], d, s_min=smin, lam=lam, rise=r, baseline=base)
        assert dec._y.data_ptr() == held.data_ptr()
        _same([dec.result(k) for k in three], a2.deconvolve(y, d, r, lam, smin, base), 'resident ' + dtype.__name__)
        assert held.cpu().numpy().tobytes() == buf.tobytes() and ref.same_bits(dec.result('baseline'), base)
    # the search: sigma=None is the trace noise, computed where the traces lie
    y = np.stack([a2.reach_trace(seed, 0.2, 300)[1] for seed in range(66)])
    held = torch.from_numpy(y).cuda()
    kinds = three + ('param', 'rss', 'target', 'status')
    for which, other in (('s_min', dict(lam=0.02)), ('lam', dict(s_min=0.1))):
        dec = TraceDeconvolver(held, d, rise=r, constrain=which, rounds=8, **other)
        want = a2.host_constrained(L, y, d, r, sr.WHICH[which], trace_noise(y), list(other.values())[0], 8)
        a2.same({k: dec.result(k) for k in kinds[:-2] + ('status',)}, want, which)
        sig = trace_noise(y)
        assert ref.same_bits(dec.sigma_device.cpu().numpy(), sig) and ref.same_bits(dec.result('target'), (sig * sig) * 300.0)
        numpy_in = TraceDeconvolver(y, d, rise=r, constrain=which, rounds=8, sigma=sig, **other)
        for k in kinds:
            assert ref.same_bits(numpy_in.result(k), dec.result(k)), (which, k)
    assert held.cpu().numpy().tobytes() == y.tobytes()
    a2.same({k: dec.result(k)[:4] for k in kinds}, a2.constrained(y[:4], d, r, sr.LAM, sig[:4], 0.1, 8), 'oracle rows', kinds)
    # scalars; one trace of one frame
    dec = TraceDeconvolver(np.array([[2.0]]), d, rise=r, lam=0.5)
    assert dec.result('calcium').tolist() == [[1.5]] and dec.result('spikes').tobytes() == np.zeros(1).tobytes() and dec.result('pools').tolist() == [1]


def test_without_a_rise_time_the_bits_stay(L):
    from deep_calcium_amd import TraceDeconvolver
    y = _traces(70, 130, 5).astype(np.float32)
    lam, smin = _penalties(70, 5)
    g = math.exp(-1.0 / 8)
    dec = TraceDeconvolver(y, g, s_min=smin, lam=lam, rise=None)
    _same([dec.result(k) for k in ('calcium', 'spikes', 'pools')], ref.deconvolve(y, g, lam, smin), 'rise=None')


def test_deconvolve_traces_device_with_a_rise_time(L, tmp_path):
    """A small recording (_pair_ref.scene 'two'): dF/F by dff_traces_device, then the oracle, against the one call with tau_rise=,
    with a numeric k and with the threshold searched."""
    from deep_calcium_amd import ar1_gamma, deconvolve_traces_device, dff_traces_device, trace_noise
    frames, _, left, right, _ = pair_ref.scene('two', 2)
    path = str(tmp_path / 'two.npz')
    np.savez(path, series_raw=frames)
    rois = [left, right]
    window, fps, tau, tau_rise, k = 101, 16.0, 0.5, 0.1, 2.0
    d, r = ar1_gamma(tau, fps), ar1_gamma(tau_rise, fps)
    dff = dff_traces_device(path, rois, window, percentile=20)
    sig = trace_noise(dff)
    want = a2.deconvolve(dff, d, r, 0.05, k * sig)
    c, s, info = deconvolve_traces_device(path, rois, window=window, tau=tau, tau_rise=tau_rise, fps=fps, k=k, lam=0.05, percentile=20, details=True)
    assert ref.same_bits(c, want[0]) and ref.same_bits(s, want[1])
    assert info['g'] == d and info['rise'] == r and ref.same_bits(info['sigma'], sig)
    assert ((s > 0).sum(1) >= 1).all()
    c, s, info = deconvolve_traces_device(path, rois, window=window, tau=tau, tau_rise=tau_rise, fps=fps, k='noise', lam=0.02, percentile=20,
                                          details=True)
    want = a2.constrained(dff, d, r, sr.SMIN, sig, 0.02, 24)
    assert ref.same_bits(c, want['calcium']) and ref.same_bits(s, want['spikes'])
    assert ref.same_bits(info['s_min'], want['param']) and ref.same_bits(info['rss'], want['rss']) and ref.same_bits(info['search_status'], want['status'])


def test_example_traces_command_with_spike_rise(L, tmp_path, monkeypatch, caplog):
    """examples/neurons/unet2ds_nf.py `traces --dff W --deconvolve TAU --fps F --spike-rise TAU_RISE --spike-k K`: `calcium` and
    `deconvolved` beside `traces`, equal to dff_traces_device followed by the oracle; the prediction is stood in for by the planted
    mask.  The log names the roots, the coefficients and the frame of the peak."""
    import importlib.util
    import logging
    import os
    from deep_calcium_amd import UNet2DSummary, ar1_gamma, dff_traces_device, hdf5_min, trace_noise
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
        spec = importlib.util.spec_from_file_location('example_unet2ds_nf_ar2', script)
        example = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(example)
    finally:
        np.random.set_state(state)
    monkeypatch.setattr(UNet2DSummary, 'predict', lambda self, dspaths, **kw: ([mask2d], ['two']))
    dff = dff_traces_device(path, mask2d.round().astype(np.uint8), 101, percentile=20)
    assert dff.shape == (2, frames.shape[0])
    d, r = ar1_gamma(0.5, 16.0), ar1_gamma(0.1, 16.0)
    want = a2.deconvolve(dff, d, r, 0.0, 2.0 * trace_noise(dff))
    cp = str(tmp_path / 'cp')
    with caplog.at_level(logging.INFO):
        example.traces([path], None, cp, dff=101, percentile=20, deconvolve=0.5, fps=16.0, spike_k=2.0, spike_rise=0.1)
    with hdf5_min.File(os.path.join(cp, 'two_traces.hdf5')) as f:
        assert f['traces'].read().tobytes() == dff.tobytes()
        assert ref.same_bits(f['calcium'].read(), want[0]) and ref.same_bits(f['deconvolved'].read(), want[1])
    g1, g2 = a2.coefficients(d, r)
    assert 'd = %.6f, r = %.6f, g1 = %.6f, g2 = %.6f' % (d, r, g1, g2) in caplog.text and 'peaks at frame' in caplog.text
    want = a2.constrained(dff, d, r, sr.SMIN, trace_noise(dff), 0.0, 24)
    cp = str(tmp_path / 'cp_searched')
    example.traces([path], None, cp, dff=101, percentile=20, deconvolve=0.5, fps=16.0, spike_constrain='s_min', spike_rise=0.1)
    with hdf5_min.File(os.path.join(cp, 'two_traces.hdf5')) as f:
        assert ref.same_bits(f['calcium'].read(), want['calcium']) and ref.same_bits(f['deconvolved'].read(), want['spikes'])
    for kw, what in ((dict(dff=101, deconvolve='auto', spike_rise=0.1), 'needs --deconvolve TAU'),
                     (dict(dff=101, deconvolve=0.5, fps=16.0, spike_rise=0.1, spike_baseline='fit'), 'not built for AR'),
                     (dict(dff=101, deconvolve=0.5, fps=16.0, spike_rise=0.5), 'shorter than the decay'),
                     (dict(dff=101, deconvolve=0.5, fps=16.0, spike_rise=0.0), 'tau and fps')):
        with pytest.raises(ValueError, match=what):
            example.traces([path], None, str(tmp_path / 'cp_err'), **kw)
