"""The noise-constrained search on the device: dc_trace_deconv_ar1_constrained against the plain-Python oracle
(tests/_deconv_search_ref.py) in every bit of param, rss, status, target, calcium, spikes and pools -- ragged workgroups of traces,
ragged folds of frames, padded rows, both input types, both parameters, one decay or one per trace, the three statuses side by
side in a wave, more traces than the residual kernel has workgroups, buffers pre-filled with canaries -- and TraceDeconvolver
(constrain=) on top of it."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _deconv_ref as ref               # noqa: E402
import _deconv_search_ref as sr         # noqa: E402

GAMMAS = (math.exp(-1.0 / 2), math.exp(-1.0 / 8), math.exp(-1.0 / 30))
CANARY = -77.25
GUARD = 5                               # canary elements / rows behind every output


@pytest.fixture(scope='module')
def L(dclib):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return dclib


def _mixed(R, T, seed):
    """Rows in turn, so that the lanes of a wave end differently: events on noise held to their noise (status 0 where the trace
    is long enough), an all-zero row held to sigma 1 (status 2), a noiseless spike train held to sigma 0 (status 1), pure noise
    held to twice its level.  -> y float64 (R, T), sigma float64[R]."""
    rs = np.random.RandomState(seed)
    y, sigma = np.zeros((R, T)), np.zeros(R)
    t = np.arange(T)
    for r in range(R):
        kind = r % 4
        sp = rs.poisson(0.05, T) > 0
        if kind == 0:
            sigma[r] = 0.1 + 0.3 * rs.rand()
            y[r] = np.convolve(sp, np.exp(-t / 8.0))[:T] + sigma[r] * rs.standard_normal(T)
        elif kind == 1:
            sigma[r] = 1.0
        elif kind == 2:
            y[r] = np.convolve(sp, np.exp(-t / 8.0))[:T]
        else:
            y[r] = 0.25 * rs.standard_normal(T)
            sigma[r] = 0.5
    return y, sigma


def _device_run(L, y, g, which, sigma, other=0.0, rounds=6, pad=0, step_again=False):
    """dc_trace_deconv_ar1_constrained on the rows of y, stored with stride T + pad.  g: a scalar, or one decay per row (the tables
    are then dc_ar1_tables').  The padding and the workspace are pre-filled with NaN; every output is GUARD elements (rows) longer
    than it need be and pre-filled with a canary: what is not written, or written beyond row R, shows.  -> dict like the oracle's.
    step_again: afterwards one more dc_trace_deconv_search_step (last = 1) on the stacks, the state and a copy of p* that the call
    left, into canary-filled outputs of its own: -> (dict, dict of that step's param, rss and status)."""
    from deep_calcium_amd.deconv import ar1_table
    R, T = y.shape
    buf = np.full((R, T + pad), np.nan, y.dtype)
    buf[:, :T] = y
    d = torch.from_numpy(buf).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    if np.ndim(g):
        gs = torch.from_numpy(np.ascontiguousarray(g, np.float64)).cuda()
        G = torch.full((R, T + 2), float('nan'), dtype=torch.float64, device='cuda')
        L.dc_ar1_tables(gs.data_ptr(), R, T, G.data_ptr(), T + 2, stream)
        gv, gp, ldG = 0.0, gs.data_ptr(), T + 2
    else:
        G = torch.from_numpy(ar1_table(g, T)).cuda()
        gv, gp, ldG = float(g), None, 0
    dsig = torch.from_numpy(np.broadcast_to(np.asarray(sigma, np.float64), (R,)).copy()).cuda()
    doth = torch.from_numpy(np.broadcast_to(np.asarray(other, np.float64), (R,)).copy()).cuda()
    assert L.dc_trace_deconv_search_state_bytes(R) == 40 * R and L.dc_trace_deconv_search_state_bytes(0) == 0
    ws = torch.full((3 * R * T + GUARD,), float('nan'), dtype=torch.float64, device='cuda')
    ws[3 * R * T:] = CANARY
    state = torch.full((5 * R + GUARD,), CANARY, dtype=torch.float64, device='cuda')
    c = torch.full((R + GUARD, T), CANARY, dtype=torch.float64, device='cuda')
    s = torch.full((R + GUARD, T), CANARY, dtype=torch.float64, device='cuda')
    n = torch.full((R + GUARD,), -7, dtype=torch.int32, device='cuda')
    param = torch.full((R + GUARD,), CANARY, dtype=torch.float64, device='cuda')
    rss = torch.full((R + GUARD,), CANARY, dtype=torch.float64, device='cuda')
    status = torch.full((R + GUARD,), -7, dtype=torch.int32, device='cuda')
    L.dc_trace_deconv_ar1_constrained(d.data_ptr(), int(y.dtype == np.float64), T + pad, R, T, gv, gp, G.data_ptr(), ldG, which, dsig.data_ptr(),
                                      doth.data_ptr(), rounds, ws.data_ptr(), state.data_ptr(), c.data_ptr(), s.data_ptr(), n.data_ptr(),
                                      param.data_ptr(), rss.data_ptr(), status.data_ptr(), stream)
    torch.cuda.synchronize()
    assert d.cpu().numpy().tobytes() == buf.tobytes()                      # read in place, never written
    for name, a in (('calcium', c), ('spikes', s), ('param', param), ('rss', rss)):
        assert (a[R:].cpu().numpy() == CANARY).all(), (name, 'written beyond row R')
    assert (n[R:].cpu().numpy() == -7).all() and (status[R:].cpu().numpy() == -7).all()
    assert (ws[3 * R * T:].cpu().numpy() == CANARY).all() and (state[5 * R:].cpu().numpy() == CANARY).all()
    out = dict(param=param[:R].cpu().numpy(), rss=rss[:R].cpu().numpy(), status=status[:R].cpu().numpy(), target=state[3 * R:4 * R].cpu().numpy(),
               calcium=c[:R].cpu().numpy(), spikes=s[:R].cpu().numpy(), pools=n[:R].cpu().numpy())
    if not step_again:
        return out
    p2, before = param.clone(), ws.clone()
    r2 = torch.full((R + GUARD,), CANARY, dtype=torch.float64, device='cuda')
    s2 = torch.full((R + GUARD,), -7, dtype=torch.int32, device='cuda')
    L.dc_trace_deconv_search_step(d.data_ptr(), int(y.dtype == np.float64), T + pad, R, T, G.data_ptr(), ldG, ws.data_ptr(), n.data_ptr(), 1,
                                  state.data_ptr(), p2.data_ptr(), r2.data_ptr(), s2.data_ptr(), stream)
    torch.cuda.synchronize()
    assert (p2[R:].cpu().numpy() == CANARY).all() and (r2[R:].cpu().numpy() == CANARY).all() and (s2[R:].cpu().numpy() == -7).all()
    assert ws.cpu().numpy().tobytes() == before.cpu().numpy().tobytes() and (state[5 * R:].cpu().numpy() == CANARY).all()
    return out, dict(param=p2[:R].cpu().numpy(), rss=r2[:R].cpu().numpy(), status=s2[:R].cpu().numpy())


SEVEN = sr.NAMES + ('target',)


def _same(got, want, what, names=SEVEN):
    for name in names:
        a, b = got[name], want[name]
        assert ref.same_bits(a, b), (name, what, np.argwhere(a != b)[:5].tolist())


@pytest.mark.parametrize('T', (1, 3, 63, 64, 65, 255, 257, 600))
@pytest.mark.parametrize('R', (1, 63, 65, 130))
def test_device_equals_the_oracle_bit_for_bit(L, R, T):
    """Ragged workgroups of the forward kernel (64 traces) and ragged folds (256 lanes), padded rows (ld = T + 3), float32 and
    float64, both parameters with the other one fixed above zero, one decay for all and one per trace (the oracle then runs every
    row with its own table)."""
    seed = 1000 * R + T
    y64, sigma = _mixed(R, T, seed)
    g_each = np.array([GAMMAS[(r // 4 + T) % 3] for r in range(R)])
    rounds = 5 if R * T > 20000 else 9
    for dtype, pad, which, g, other in ((np.float32, 3, sr.SMIN, GAMMAS[(R + T) % 3], 0.0), (np.float64, 0, sr.LAM, g_each, 0.0),
                                        (np.float64, 3, sr.SMIN, g_each, 0.05), (np.float32, 0, sr.LAM, GAMMAS[1], 0.1)):
        y = y64.astype(dtype)
        want = sr.deconvolve(y, g, which, sigma, other, rounds)
        got = _device_run(L, y, g, which, sigma, other, rounds, pad=pad)
        _same(got, want, (R, T, dtype.__name__, pad, which, np.ndim(g)))


def test_the_three_statuses_side_by_side_in_one_wave(L):
    """Zero rows (never bracketed), noiseless rows (finished after round 0) and reach rows (bracketed) interleaved in the 64 lanes
    of one forward workgroup: every row gives what it gives alone."""
    from deep_calcium_amd.deconv import trace_noise
    T, g, rounds = 1024, GAMMAS[1], 24
    rows, sigma = [], []
    for i in range(22):
        sp, y = ref.reach_trace(i, 0.3, T)
        rows += [np.zeros(T, np.float32), np.convolve(sp, np.exp(-np.arange(T) / 8.0))[:T].astype(np.float32), y]
        sigma += [1.0, 0.0, float(trace_noise(y[None])[0])]
    y, sigma = np.stack(rows[:64]), np.array(sigma[:64])
    got = _device_run(L, y, g, sr.SMIN, sigma, 0.0, rounds)
    assert got['status'].tolist() == ([2, 1, 0] * 22)[:64]
    assert (got['param'][0::3] == 2.0 ** (rounds - 1)).all() and (got['rss'][0::3] == 0).all() and (got['param'][1::3] == 0).all()
    want = sr.host_entry(L, y, g, sr.SMIN, sigma, 0.0, rounds)              # dc_trace_deconv_ar1_constrained_host, itself equal to the oracle (test_deconv_search_api.py)
    _same(got, want, 'mixed wave', sr.NAMES)
    for r in (0, 1, 2, 61, 62, 63):
        alone = sr.deconvolve(y[r:r + 1], g, sr.SMIN, sigma[r:r + 1], 0.0, rounds)
        _same({k: v[r:r + 1] for k, v in got.items()}, alone, ('alone', r))
    assert (got['rss'][2::3] <= got['target'][2::3]).all()


@pytest.mark.parametrize('each', (False, True))
def test_one_residual_and_step_launch_alone(L, each):
    """dc_trace_deconv_search_step after a finished search: the stacks in the workspace are those of the final pass at p*, so the
    residual it folds is RSS(p*) = rss and the step it takes keeps the bracket's lower end: p*, rss and the status come out again,
    bit for bit, for bracketed, finished and never-bracketed traces alike."""
    R, T = 70, 300
    y64, sigma = _mixed(R, T, 9)
    g = np.array([GAMMAS[r % 3] for r in range(R)]) if each else GAMMAS[1]
    got, again = _device_run(L, y64.astype(np.float32), g, sr.SMIN, sigma, 0.0, 7, pad=3, step_again=True)
    assert set(got['status'].tolist()) == {0, 1, 2}
    _same(again, got, ('step alone', each), ('param', 'rss', 'status'))
    _same(got, sr.deconvolve(y64.astype(np.float32), g, sr.SMIN, sigma, 0.0, 7), ('step alone: the search itself', each))


def test_more_traces_than_residual_workgroups(L):
    """Beyond DC_TRACE_DECONV_SEARCH_MAX_GROUPS = 8192 traces a workgroup of the residual kernel walks several."""
    R, T, rounds = 8192 + 70, 5, 3
    y64, sigma = _mixed(R, T, 5)
    y = y64.astype(np.float32)
    got = _device_run(L, y, GAMMAS[1], sr.SMIN, sigma, 0.0, rounds, pad=1)
    want = sr.host_entry(L, y, GAMMAS[1], sr.SMIN, sigma, 0.0, rounds)
    _same(got, want, 'capped grid', sr.NAMES)
    rows = [0, 1, 2, 3, 8191, 8192, 8193, R - 1]
    _same({k: v[rows] for k, v in got.items()}, sr.deconvolve(y[rows], GAMMAS[1], sr.SMIN, sigma[rows], 0.0, rounds), 'oracle rows')


def test_trace_deconvolver_constrained(L):
    """sigma=None on a resident tensor is the trace noise, computed where the traces lie: the bits of passing trace_noise(y).  The
    input tensor is not written; numpy input gives the same; a decay per trace and 'lam' go through the same object."""
    from deep_calcium_amd import TraceDeconvolver
    from deep_calcium_amd.deconv import trace_noise
    y = np.stack([ref.reach_trace(seed, 0.3, 600)[1] for seed in range(70)])
    g = GAMMAS[1]
    d = torch.from_numpy(y).cuda()
    auto = TraceDeconvolver(d, g, constrain='s_min', rounds=8)
    given = TraceDeconvolver(d, g, constrain='s_min', sigma=trace_noise(y), rounds=8)
    on_dev = TraceDeconvolver(y, g, constrain='s_min', sigma=torch.from_numpy(trace_noise(y)).cuda(), rounds=8)
    kinds = ('calcium', 'spikes', 'pools', 'param', 'rss', 'target', 'status')
    for kind in kinds:
        assert ref.same_bits(auto.result(kind), given.result(kind)) and ref.same_bits(auto.result(kind), on_dev.result(kind)), kind
    assert d.cpu().numpy().tobytes() == y.tobytes()
    assert ref.same_bits(auto.sigma_device.cpu().numpy(), trace_noise(y))
    assert auto.result('param').dtype == np.float64 and auto.result('status').dtype == np.int32 and auto.result_device('rss').is_cuda
    want = sr.deconvolve(y[:6], g, sr.SMIN, trace_noise(y[:6]), 0.0, 8)
    _same({k: auto.result(k)[:6] for k in kinds}, want, 'TraceDeconvolver')
    assert (auto.result('status') == 0).all()
    g_each = np.array([GAMMAS[r % 3] for r in range(70)])
    each = TraceDeconvolver(d, g_each, lam=0.0, s_min=0.1, constrain='lam', rounds=5)
    want = sr.deconvolve(y[:6], g_each[:6], sr.LAM, trace_noise(y[:6]), 0.1, 5)
    _same({k: each.result(k)[:6] for k in kinds}, want, 'TraceDeconvolver, lam, each')


def test_unconstrained_path_gives_the_bits_it_gave(L):
    from deep_calcium_amd import TraceDeconvolver
    from deep_calcium_amd.deconv import trace_noise
    y = np.stack([ref.reach_trace(seed, 0.2, 300)[1] for seed in range(66)])
    smin = 2.0 * trace_noise(y)
    dec = TraceDeconvolver(y, GAMMAS[1], s_min=smin, lam=0.05)
    want = ref.host_entry(L, y, GAMMAS[1], 0.05, smin)
    for kind, b in zip(('calcium', 'spikes', 'pools'), want):
        assert ref.same_bits(dec.result(kind), b), kind
    for kind in ('param', 'rss', 'target', 'status'):
        with pytest.raises(ValueError, match='is not one of calcium, spikes, pools'):
            dec.result(kind)


def test_deconvolve_traces_device_with_the_threshold_searched(L, tmp_path):
    """k='noise' end to end on a small recording (_pair_ref.scene 'two'): dF/F by dff_traces_device, then the oracles -- the noise,
    the estimate, pick_gamma, the search -- against the one call, for a given tau, 'auto' and 'each'; a numeric k gives no new keys."""
    import _dyn_ref as dyn_ref
    import _pair_ref as pair_ref
    from deep_calcium_amd import ar1_gamma, deconvolve_traces_device, dff_traces_device, pick_gamma
    frames, _, left, right, _ = pair_ref.scene('two', 2)
    path = str(tmp_path / 'two.npz')
    np.savez(path, series_raw=frames)
    rois, window = [left, right], 101
    dff = dff_traces_device(path, rois, window, percentile=20)
    sigma, _, g_raw = dyn_ref.estimate(dff, 5)
    g_each, _, g_pool = pick_gamma(g_raw)
    for tau, fps, g in ((0.5, 16.0, np.full(2, ar1_gamma(0.5, 16.0))), ('auto', None, np.full(2, g_pool)), ('each', None, g_each)):
        c, s, info = deconvolve_traces_device(path, rois, window=window, tau=tau, fps=fps, k='noise', lam=0.02, percentile=20, details=True)
        want = sr.deconvolve(dff, g, sr.SMIN, sigma, 0.02, 24)
        assert ref.same_bits(c, want['calcium']) and ref.same_bits(s, want['spikes']), tau
        assert sorted(info) == ['g', 'g_raw', 'pooled', 'rss', 's_min', 'search_status', 'sigma', 'status']
        assert ref.same_bits(info['s_min'], want['param']) and ref.same_bits(info['rss'], want['rss']), tau
        assert ref.same_bits(info['search_status'], want['status']) and ref.same_bits(info['sigma'], sigma), tau
        two = deconvolve_traces_device(path, rois, window=window, tau=tau, fps=fps, k='noise', lam=0.02, percentile=20)
        assert len(two) == 2 and ref.same_bits(two[0], c) and ref.same_bits(two[1], s)
    info = deconvolve_traces_device(path, rois, window=window, tau='auto', k=2.0, percentile=20, details=True)[2]
    assert sorted(info) == ['g', 'g_raw', 'pooled', 'sigma', 'status']
