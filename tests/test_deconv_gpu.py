"""Spikes by deconvolution on the device: dc_trace_deconv_ar1 against the plain-Python oracle (tests/_deconv_ref.py), or the library's
host entry point dc_trace_deconv_ar1_host where the oracle would be slow, in every bit of calcium, spikes and pools -- ragged
tiles of traces and frames, padded rows, both input types, per-trace penalties, divergent lanes, buffers pre-filled with NaN -- and
TraceDeconvolver / deconvolve_traces_device on top of it."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _deconv_ref as ref       # noqa: E402
import _pair_ref as pair_ref    # noqa: E402

LANES = 64                      # traces per workgroup of the forward kernel
FRAMES = 64                     # frames per staged tile
GAMMAS = (math.exp(-1.0 / 2), math.exp(-1.0 / 8), math.exp(-1.0 / 30))


@pytest.fixture(scope='module')
def L(dclib):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return dclib


def _traces(R, T, seed):
    """Rows in turn: events on noise, pure noise around zero, a drifting trace with large values, and the three structural
    traces -- the ramp (the stack reaches depth T), the collapse (one pool) and the cascade -- so that neighbouring lanes of a
    wave diverge."""
    rs = np.random.RandomState(seed)
    y = np.empty((R, T))
    t = np.arange(T)
    for r in range(R):
        kind = r % 6
        if kind == 0:
            sp = rs.poisson(0.05, T) > 0
            y[r] = np.convolve(sp, np.exp(-t / 8.0))[:T] + 0.2 * rs.standard_normal(T)
        elif kind == 1:
            y[r] = 0.5 * rs.standard_normal(T)
        elif kind == 2:
            y[r] = 100.0 * np.cumsum(rs.standard_normal(T)) / np.sqrt(T) + 3.0
        elif kind == 3:
            y[r] = t + 1.0
        elif kind == 4:
            y[r] = -1.0 * t
        else:
            y[r] = np.where(t < T - 1, t + 1.0, -1e6)
    return y


def _penalties(R, seed):
    """lam and s_min that differ from row to row, zeros included; none for the ramps, which then keep every pool."""
    rs = np.random.RandomState(seed + 1)
    lam = np.where(rs.rand(R) < 0.5, 0.0, 0.3 * rs.rand(R))
    smin = np.where(rs.rand(R) < 0.4, 0.0, 0.8 * rs.rand(R))
    lam[3::6] = smin[3::6] = 0.0
    return lam, smin


def _device_run(L, y, g, lam, smin, pad=0, check_input=True):
    """dc_trace_deconv_ar1 on the rows of y, stored with stride T + pad.  The padding, the outputs and the workspace are
    pre-filled with NaN (pools with -1): an element that is not written, or padding that is read, shows.  -> calcium, spikes, pools."""
    from deep_calcium_amd.deconv import ar1_table
    R, T = y.shape
    buf = np.full((R, T + pad), np.nan, y.dtype)
    buf[:, :T] = y
    d = torch.from_numpy(buf).cuda()
    G = torch.from_numpy(ar1_table(g, T)).cuda()
    dl = torch.from_numpy(np.broadcast_to(np.asarray(lam, np.float64), (R,)).copy()).cuda()
    ds = torch.from_numpy(np.broadcast_to(np.asarray(smin, np.float64), (R,)).copy()).cuda()
    nbytes = L.dc_trace_deconv_ws_bytes(R, T)
    assert nbytes == 24 * R * T
    ws = torch.full((nbytes // 8,), float('nan'), dtype=torch.float64, device='cuda')
    c = torch.full((R, T), float('nan'), dtype=torch.float64, device='cuda')
    s = torch.full((R, T), float('nan'), dtype=torch.float64, device='cuda')
    n = torch.full((R,), -1, dtype=torch.int32, device='cuda')
    L.dc_trace_deconv_ar1(d.data_ptr(), int(y.dtype == np.float64), T + pad, R, T, float(g), G.data_ptr(), dl.data_ptr(), ds.data_ptr(),
                          ws.data_ptr(), c.data_ptr(), s.data_ptr(), n.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if check_input:
        assert d.cpu().numpy().tobytes() == buf.tobytes()                  # read in place, never written
    return c.cpu().numpy(), s.cpu().numpy(), n.cpu().numpy()


def _same(got, want, what):
    for name, a, b in zip(('calcium', 'spikes', 'pools'), got, want):
        assert not np.isnan(a).any() if a.dtype.kind == 'f' else (a >= 1).all(), (name, what)
        assert ref.same_bits(a, b), (name, what, np.argwhere(a != b)[:5].tolist())


@pytest.mark.parametrize('T', (1, 2, FRAMES - 1, FRAMES, FRAMES + 1, 257))
@pytest.mark.parametrize('R', (1, LANES - 1, LANES, LANES + 1, 130))
def test_device_equals_the_oracle_bit_for_bit(L, R, T):
    """Ragged tiles in both directions, padded rows (ld = T + 3), float32 and float64 traces, penalties that differ from row to
    row, and the ramp, the collapse and the cascade in lanes next to ordinary traces."""
    seed = 1000 * R + T
    g = GAMMAS[(R + T) % 3]
    y64 = _traces(R, T, seed)
    lam, smin = _penalties(R, seed)
    for dtype, pad in ((np.float32, 3), (np.float64, 0), (np.float64, 3), (np.float32, 0)):
        y = y64.astype(dtype)
        want = ref.deconvolve(y, g, lam, smin)
        _same(_device_run(L, y, g, lam, smin, pad=pad), want, (R, T, dtype.__name__, pad))
    if T > 1 and R > 5:
        assert want[2][3] == T and want[2][4] == 1                         # the ramp kept every pool, the collapse one
        assert want[0][4].tobytes() == np.zeros(T).tobytes() and want[1][4].tobytes() == np.zeros(T).tobytes()


def test_device_equals_the_host_entry_on_longer_traces_and_repeats(L):
    """Several workgroups, sixteen frame tiles, stacks hundreds deep: against dc_trace_deconv_ar1_host (itself equal to the oracle in
    tests/test_deconv_api.py); a sample of rows against the oracle as well; and a second run gives the same bits."""
    R, T = 300, 1000
    y = _traces(R, T, 77).astype(np.float32)
    lam, smin = _penalties(R, 77)
    for g in GAMMAS[1:]:
        want = ref.host_entry(L, y, g, lam, smin)
        got = _device_run(L, y, g, lam, smin, pad=3)
        _same(got, want, g)
        again = _device_run(L, y, g, lam, smin, pad=3)
        _same(again, got, 'second run')
        rows = [0, 3, 4, 5, 64, 65, 128, 255, 256, 299]
        _same([a[rows] for a in got], ref.deconvolve(y[rows], g, lam[rows], smin[rows]), 'oracle rows')
    assert got[2].max() == T and got[2].min() == 1


def test_uniform_scalar_penalties_and_reach_traces(L):
    """The traces of the reach table (sigma 0.3), s_min = 3 sigma_hat per trace: the device finds the events the oracle finds."""
    from deep_calcium_amd.deconv import trace_noise
    y = np.stack([ref.reach_trace(seed, 0.3)[1] for seed in range(8)])
    smin = 3.0 * trace_noise(y)
    g = GAMMAS[1]
    want = ref.deconvolve(y, g, 0.0, smin)
    got = _device_run(L, y, g, 0.0, smin)
    _same(got, want, 'reach')
    assert ((got[1] > 0).sum(1) > 5).all()


def test_trace_deconvolver_numpy_and_resident_input(L):
    from deep_calcium_amd import TraceDeconvolver
    R, T = 70, 130
    y64 = _traces(R, T, 5)
    lam, smin = _penalties(R, 5)
    g = GAMMAS[1]
    for dtype in (np.float32, np.float64):
        y = y64.astype(dtype)
        want = ref.deconvolve(y, g, lam, smin)
        dec = TraceDeconvolver(y, g, s_min=smin, lam=lam)
        assert dec.result('calcium').dtype == np.float64 and dec.result('pools').dtype == np.int32
        _same([dec.result(k) for k in ('calcium', 'spikes', 'pools')], want, dtype.__name__)
        assert dec.result_device('spikes') is dec.result_device('spikes') and dec.result_device('calcium').is_cuda      # run once
        # a resident tensor with padded rows: read in place and left unchanged
        buf = np.full((R, T + 3), np.nan, dtype)
        buf[:, :T] = y
        d = torch.from_numpy(buf).cuda()
        view = d[:, :T]
        assert view.stride(0) == T + 3
        dec = TraceDeconvolver(view, g, s_min=smin, lam=lam)
        assert dec._y.data_ptr() == d.data_ptr()
        _same([dec.result(k) for k in ('calcium', 'spikes', 'pools')], want, 'resident ' + dtype.__name__)
        assert d.cpu().numpy().tobytes() == buf.tobytes()
    # scalars; one trace of one frame
    dec = TraceDeconvolver(y64.astype(np.float32), g, s_min=0.25, lam=0.1)
    _same([dec.result(k) for k in ('calcium', 'spikes', 'pools')], ref.deconvolve(y64.astype(np.float32), g, 0.1, 0.25), 'scalars')
    dec = TraceDeconvolver(np.array([[2.0]]), g, lam=0.5)
    assert dec.result('calcium').tolist() == [[1.5]] and dec.result('spikes').tobytes() == np.zeros(1).tobytes() and dec.result('pools').tolist() == [1]
    with pytest.raises(ValueError, match='not one of'):
        dec.result('events')
    with pytest.raises(ValueError, match='rows of a device tensor must be contiguous'):
        TraceDeconvolver(torch.zeros((8, 4), device='cuda').t(), g)
    with pytest.raises(ValueError, match='float32 or float64'):
        TraceDeconvolver(torch.zeros((4, 8), dtype=torch.int64, device='cuda'), g)


def test_deconvolve_traces_device_end_to_end(L, tmp_path):
    """A small recording (_pair_ref.scene 'two': two cells side by side with independent activity): dF/F by dff_traces_device, then
    the oracle, against the one call -- and a TraceDeconvolver fed by TraceBaseline.result_device('dff') where it lies."""
    from deep_calcium_amd import TraceBaseline, TraceDeconvolver, ar1_gamma, deconvolve_traces_device, dff_traces_device, extract_traces_device, trace_noise
    frames, _, left, right, _ = pair_ref.scene('two', 2)
    path = str(tmp_path / 'two.npz')
    np.savez(path, series_raw=frames)
    rois = [left, right]
    window, fps, tau, k = 101, 16.0, 0.5, 2.0
    g = ar1_gamma(tau, fps)
    dff = dff_traces_device(path, rois, window, percentile=20)
    assert dff.dtype == np.float32 and dff.shape == (2, frames.shape[0])
    want = ref.deconvolve(dff, g, 0.05, k * trace_noise(dff))
    c, s = deconvolve_traces_device(path, rois, window=window, tau=tau, fps=fps, k=k, lam=0.05, percentile=20)
    assert ref.same_bits(c, want[0]) and ref.same_bits(s, want[1])
    assert ((s > 0).sum(1) >= 2).all()                                       # both cells fire in this scene
    tb = TraceBaseline(extract_traces_device(path, rois, kind='sum'), [len(left), len(right)], window, percentile=20)
    dec = TraceDeconvolver(tb.result_device('dff'), g, s_min=k * trace_noise(tb.result('dff')), lam=0.05)
    assert ref.same_bits(dec.result('calcium'), want[0]) and ref.same_bits(dec.result('spikes'), want[1])
    assert np.array_equal(dec.result('pools'), want[2])


def test_example_traces_command_with_deconvolve(L, tmp_path, monkeypatch):
    """examples/neurons/unet2ds_nf.py `traces --dff W --deconvolve TAU --fps F --spike-k K`: `calcium` and `deconvolved` beside
    `traces`, equal to dff_traces_device followed by the oracle; the prediction is stood in for by the planted mask."""
    import importlib.util
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
        spec = importlib.util.spec_from_file_location('example_unet2ds_nf_deconv', script)
        example = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(example)
    finally:
        np.random.set_state(state)
    monkeypatch.setattr(UNet2DSummary, 'predict', lambda self, dspaths, **kw: ([mask2d], ['two']))
    dff = dff_traces_device(path, mask2d.round().astype(np.uint8), 101, percentile=20)
    assert dff.shape == (2, frames.shape[0])
    want = ref.deconvolve(dff, ar1_gamma(0.5, 16.0), 0.0, 2.0 * trace_noise(dff))
    cp = str(tmp_path / 'cp')
    example.traces([path], None, cp, dff=101, percentile=20, deconvolve=0.5, fps=16.0, spike_k=2.0)
    with hdf5_min.File(os.path.join(cp, 'two_traces.hdf5')) as f:
        assert f['traces'].read().tobytes() == dff.tobytes()
        assert ref.same_bits(f['calcium'].read(), want[0]) and ref.same_bits(f['deconvolved'].read(), want[1])
    for kw, what in ((dict(deconvolve=0.5, fps=16.0), 'needs --dff'), (dict(dff=101, deconvolve=0.5), 'needs --fps'),
                     (dict(dff=101, deconvolve=0.5, fps=16.0, spike_k=-1.0), 'K >= 0'), (dict(dff=101, deconvolve=0.0, fps=16.0), 'tau and fps')):
        with pytest.raises(ValueError, match=what):
            example.traces([path], None, str(tmp_path / 'cp_err'), **kw)
