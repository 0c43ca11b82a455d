"""A baseline in the deconvolution on the device: dc_trace_deconv_ar1_base, dc_trace_deconv_ar1_fit_base and
dc_trace_deconv_ar1_constrained_base against the plain-Python oracle (tests/_deconv_base_ref.py) in every bit of calcium, spikes,
pools, param, baseline, rss, status and target -- ragged workgroups of traces, ragged folds of frames, padded rows, both input types,
both parameters, one decay or one per trace, the three statuses side by side in a wave, more traces than the residual kernel has
workgroups, buffers pre-filled with canaries --, one dc_trace_deconv_base_step launch alone, and TraceDeconvolver(baseline=) and
deconvolve_traces_device(baseline=) on top of them."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _deconv_base_ref as br           # noqa: E402
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
    """Rows in turn, so that the lanes of a wave end differently: events on noise above an offset held to their noise (status 0
    where the trace is long enough), an all-zero row held to sigma 1 (status 2), a noiseless spike train held to sigma 0 (status
    1), pure noise around an offset held to twice its level.  -> y float64 (R, T), sigma float64[R]."""
    rs = np.random.RandomState(seed)
    y, sigma = np.zeros((R, T)), np.zeros(R)
    t = np.arange(T)
    for r in range(R):
        kind = r % 4
        sp = rs.poisson(0.05, T) > 0
        if kind == 0:
            sigma[r] = 0.1 + 0.3 * rs.rand()
            y[r] = np.convolve(sp, np.exp(-t / 8.0))[:T] + sigma[r] * (rs.standard_normal(T) + 1.0)
        elif kind == 1:
            sigma[r] = 1.0
        elif kind == 2:
            y[r] = np.convolve(sp, np.exp(-t / 8.0))[:T]
        else:
            y[r] = 0.25 * rs.standard_normal(T) - 0.2
            sigma[r] = 0.5
    return y, sigma


class _Device(object):
    """The rows of y on the device with stride T + pad, the padding and the workspace pre-filled with NaN; every output GUARD
    elements (rows) longer than it need be and pre-filled with a canary: what is not written, or written beyond row R, shows.
    g: a scalar, or one decay per row (the tables are then dc_ar1_tables')."""

    def __init__(self, L, y, g, pad=0):
        from deep_calcium_amd.deconv import ar1_table
        self.L, self.y = L, y
        R, T = self.R, self.T = y.shape
        self.ld, self.f64 = T + pad, int(y.dtype == np.float64)
        self.buf = np.full((R, T + pad), np.nan, y.dtype)
        self.buf[:, :T] = y
        self.d = torch.from_numpy(self.buf).cuda()
        self.stream = torch.cuda.current_stream().cuda_stream
        if np.ndim(g):
            self.gs = torch.from_numpy(np.ascontiguousarray(g, np.float64)).cuda()
            self.G = torch.full((R, T + 2), float('nan'), dtype=torch.float64, device='cuda')
            L.dc_ar1_tables(self.gs.data_ptr(), R, T, self.G.data_ptr(), T + 2, self.stream)
            self.gv, self.gp, self.ldG = 0.0, self.gs.data_ptr(), T + 2
        else:
            self.G = torch.from_numpy(ar1_table(g, T)).cuda()
            self.gv, self.gp, self.ldG = float(g), None, 0
        self.ws = torch.full((3 * R * T + GUARD,), float('nan'), dtype=torch.float64, device='cuda')
        self.ws[3 * R * T:] = CANARY
        self.c, self.s = self.full((R + GUARD, T)), self.full((R + GUARD, T))
        self.n = self.full(R + GUARD, torch.int32)

    def full(self, shape, dtype=torch.float64):
        return torch.full(shape if isinstance(shape, tuple) else (shape,), -7 if dtype == torch.int32 else CANARY, dtype=dtype, device='cuda')

    def vector(self, x, guard=False):
        a = np.broadcast_to(np.asarray(x, np.float64), (self.R,)).copy()
        return torch.from_numpy(np.concatenate([a, np.full(GUARD, CANARY)]) if guard else a).cuda()

    def check(self, **more):
        """Synchronise; the input was not written and nothing lies beyond row R.  -> the three outputs as numpy."""
        torch.cuda.synchronize()
        R, T = self.R, self.T
        assert self.d.cpu().numpy().tobytes() == self.buf.tobytes()
        for name, a in dict(calcium=self.c, spikes=self.s, **more).items():
            tail = a[R:].cpu().numpy()
            assert (tail == (-7 if a.dtype == torch.int32 else CANARY)).all(), (name, 'written beyond row R')
        assert (self.n[R:].cpu().numpy() == -7).all() and (self.ws[3 * R * T:].cpu().numpy() == CANARY).all()
        return dict(calcium=self.c[:R].cpu().numpy(), spikes=self.s[:R].cpu().numpy(), pools=self.n[:R].cpu().numpy())

    def given(self, lam, smin, base):
        """dc_trace_deconv_ar1_base -> dict like the oracle's deconvolve()."""
        lam, smin, b = self.vector(lam), self.vector(smin), self.vector(base, True)
        before = b.clone()
        self.L.dc_trace_deconv_ar1_base(self.d.data_ptr(), self.f64, self.ld, self.R, self.T, self.gv, self.gp, self.G.data_ptr(), self.ldG,
                                        lam.data_ptr(), smin.data_ptr(), b.data_ptr(), self.ws.data_ptr(), self.c.data_ptr(), self.s.data_ptr(),
                                        self.n.data_ptr(), self.stream)
        out = self.check()
        assert b.cpu().numpy().tobytes() == before.cpu().numpy().tobytes()          # read, never written
        out['baseline'] = b[:self.R].cpu().numpy()
        return out

    def fit(self, lam, smin, base, rounds):
        """dc_trace_deconv_ar1_fit_base -> dict like the oracle's deconvolve()."""
        lam, smin, b = self.vector(lam), self.vector(smin), self.vector(base, True)
        self.L.dc_trace_deconv_ar1_fit_base(self.d.data_ptr(), self.f64, self.ld, self.R, self.T, self.gv, self.gp, self.G.data_ptr(), self.ldG,
                                            lam.data_ptr(), smin.data_ptr(), rounds, self.ws.data_ptr(), self.c.data_ptr(), self.s.data_ptr(),
                                            self.n.data_ptr(), b.data_ptr(), self.stream)
        out = self.check(baseline=b)
        out['baseline'] = b[:self.R].cpu().numpy()
        return out

    def search(self, which, sigma, other, base, rounds):
        """dc_trace_deconv_ar1_constrained_base -> dict like the oracle's deconvolve_search()."""
        R = self.R
        assert self.L.dc_trace_deconv_base_state_bytes(R) == 56 * R and self.L.dc_trace_deconv_base_state_bytes(0) == 0
        sigma, other, b = self.vector(sigma), self.vector(other), self.vector(base, True)
        self.state = self.full(7 * R + GUARD)
        self.param, self.rss, self.status, self.base = self.full(R + GUARD), self.full(R + GUARD), self.full(R + GUARD, torch.int32), b
        self.L.dc_trace_deconv_ar1_constrained_base(self.d.data_ptr(), self.f64, self.ld, R, self.T, self.gv, self.gp, self.G.data_ptr(), self.ldG,
                                                    which, sigma.data_ptr(), other.data_ptr(), rounds, self.ws.data_ptr(), self.state.data_ptr(),
                                                    self.c.data_ptr(), self.s.data_ptr(), self.n.data_ptr(), self.param.data_ptr(), b.data_ptr(),
                                                    self.rss.data_ptr(), self.status.data_ptr(), self.stream)
        out = self.check(param=self.param, baseline=b, rss=self.rss, status=self.status)
        assert (self.state[7 * R:].cpu().numpy() == CANARY).all()
        out.update(param=self.param[:R].cpu().numpy(), baseline=b[:R].cpu().numpy(), rss=self.rss[:R].cpu().numpy(),
                   status=self.status[:R].cpu().numpy(), target=self.state[3 * R:4 * R].cpu().numpy())
        return out


EIGHT = br.SEARCH_NAMES + ('target',)


def _same(got, want, what, names):
    for name in names:
        a, b = got[name], want[name]
        assert ref.same_bits(a, b), (name, what, np.argwhere(a != b)[:5].tolist())


@pytest.mark.parametrize('T', (1, 3, 63, 64, 65, 255, 257, 600))
@pytest.mark.parametrize('R', (1, 63, 65, 130))
def test_device_equals_the_oracle_bit_for_bit(L, R, T):
    """Ragged workgroups of the forward kernel (64 traces) and ragged folds (256 lanes), padded rows (ld = T + 3), float32 and
    float64, one decay for all and one per trace: the fit at 1 and 5 rounds from a start per trace, the joint search of either
    parameter in 6 rounds with the other one fixed above zero.  Every row against the plain-Python oracle, and against the
    library's host entry points (dc_trace_deconv_ar1_fit_base_host, dc_trace_deconv_ar1_constrained_base_host), which
    test_deconv_base_api.py holds to the same oracle."""
    seed = 1000 * R + T
    y64, sigma = _mixed(R, T, seed)
    g_each = np.array([GAMMAS[(r // 4 + T) % 3] for r in range(R)])
    b0 = np.where(np.arange(R) % 3 == 0, 0.0, 0.1 * np.sin(np.arange(R)))
    for dtype, pad, g, which, other, rounds in ((np.float32, 3, GAMMAS[(R + T) % 3], br.SMIN, 0.05, 1), (np.float64, 0, g_each, br.LAM, 0.1, 5)):
        y = y64.astype(dtype)
        dev = _Device(L, y, g, pad)
        what = (R, T, dtype.__name__, pad, which, np.ndim(g))
        lam, smin = (other, 0.3 * sigma) if which == br.SMIN else (0.2 * sigma, other)
        got = dev.fit(lam, smin, b0, rounds)
        _same(got, br.host_fit(L, y, g, lam, smin, b0, rounds), ('fit',) + what, br.FIT_NAMES)
        _same(got, br.deconvolve(y, g, lam, smin, b0, rounds), ('fit, oracle',) + what, br.FIT_NAMES)
        got = dev.search(which, sigma, other, b0, 6)
        _same(got, br.host_search(L, y, g, which, sigma, other, b0, 6), ('search',) + what, br.SEARCH_NAMES)
        _same(got, br.deconvolve_search(y, g, which, sigma, other, b0, 6), ('search, oracle',) + what, EIGHT)


def test_the_three_statuses_side_by_side_in_one_wave(L):
    """Zero rows (never bracketed), noiseless rows (finished after round 0: they keep b_0) and dF/F rows (bracketed) interleaved in
    the 64 lanes of one forward workgroup: every row gives what it gives alone."""
    from deep_calcium_amd.deconv import trace_noise
    T, g, rounds = 1024, GAMMAS[1], 12
    rows, sigma = [], []
    for i in range(22):
        sp, y, _ = br.reach_dff(i, 0.3, T)
        rows += [np.zeros(T, np.float32), np.convolve(sp, np.exp(-np.arange(T) / 8.0))[:T].astype(np.float32), y]
        sigma += [1.0, 0.0, float(trace_noise(y[None])[0])]
    y, sigma = np.stack(rows[:64]), np.array(sigma[:64])
    b0 = np.full(64, 0.0)
    b0[1::3] = 0.01
    got = _Device(L, y, g).search(br.SMIN, sigma, 0.0, b0, rounds)
    assert got['status'].tolist() == ([2, 1, 0] * 22)[:64]
    assert (got['param'][0::3] == 2.0 ** (rounds - 1)).all() and (got['rss'][0::3] == 0).all() and (got['baseline'][0::3] == 0).all()
    assert (got['param'][1::3] == 0).all() and (got['baseline'][1::3] == 0.01).all()
    _same(got, br.host_search(L, y, g, br.SMIN, sigma, 0.0, b0, rounds), 'mixed wave', br.SEARCH_NAMES)
    for r in (0, 1, 2, 61, 62, 63):
        alone = br.deconvolve_search(y[r:r + 1], g, br.SMIN, sigma[r:r + 1], 0.0, b0[r:r + 1], rounds)
        _same({k: v[r:r + 1] for k, v in got.items()}, alone, ('alone', r), EIGHT)
    assert (got['rss'][2::3] <= got['target'][2::3]).all() and (got['baseline'][2::3] > 0.5 * sigma[2::3]).all()


def test_more_traces_than_residual_workgroups(L):
    """Beyond DC_TRACE_DECONV_SEARCH_MAX_GROUPS = 8192 traces a workgroup of the residual kernel walks several."""
    R, T, rounds = 8192 + 70, 5, 3
    y64, sigma = _mixed(R, T, 5)
    y = y64.astype(np.float32)
    dev = _Device(L, y, GAMMAS[1], 1)
    got = dev.search(br.SMIN, sigma, 0.0, 0.0, rounds)
    _same(got, br.host_search(L, y, GAMMAS[1], br.SMIN, sigma, 0.0, 0.0, rounds), 'capped grid', br.SEARCH_NAMES)
    rows = [0, 1, 2, 3, 8191, 8192, 8193, R - 1]
    _same({k: v[rows] for k, v in got.items()}, br.deconvolve_search(y[rows], GAMMAS[1], br.SMIN, sigma[rows], 0.0, 0.0, rounds), 'oracle rows', EIGHT)
    got = dev.fit(0.0, 0.5 * sigma, 0.0, 2)
    _same(got, br.host_fit(L, y, GAMMAS[1], 0.0, 0.5 * sigma, 0.0, 2), 'capped grid, fit', br.FIT_NAMES)


def test_a_row_stride_above_the_frames_and_a_given_baseline(L):
    """ld = T + 37 (the padding NaN) through the three entry points; the given baseline is dc_trace_deconv_ar1 on y - b precomputed
    in float64, and the baseline 0 is dc_trace_deconv_ar1 itself."""
    R, T = 67, 130
    y64, sigma = _mixed(R, T, 21)
    y = y64.astype(np.float32)
    b = 0.2 * np.cos(np.arange(R))
    dev = _Device(L, y, GAMMAS[1], 37)
    got = dev.given(0.02, 0.3 * sigma, b)
    _same(got, br.deconvolve(y, GAMMAS[1], 0.02, 0.3 * sigma, b, 0), 'given', br.FIT_NAMES)
    old = ref.host_entry(L, y.astype(np.float64) - b[:, None], GAMMAS[1], 0.02, 0.3 * sigma)
    _same(got, dict(zip(('calcium', 'spikes', 'pools'), old)), 'y - b', ('calcium', 'spikes', 'pools'))
    zero = dev.given(0.02, 0.3 * sigma, 0.0)
    _same(zero, dict(zip(('calcium', 'spikes', 'pools'), ref.host_entry(L, y, GAMMAS[1], 0.02, 0.3 * sigma))), 'b = 0', ('calcium', 'spikes', 'pools'))
    _same(dev.fit(0.02, 0.3 * sigma, b, 3), br.deconvolve(y, GAMMAS[1], 0.02, 0.3 * sigma, b, 3), 'fit, stride', br.FIT_NAMES)
    _same(dev.search(br.LAM, sigma, 0.1, b, 4), br.deconvolve_search(y, GAMMAS[1], br.LAM, sigma, 0.1, b, 4), 'search, stride', EIGHT)


@pytest.mark.parametrize('each', (False, True))
def test_one_residual_launch_alone(L, each):
    """dc_trace_deconv_base_step on the stacks a dc_trace_deconv_ar1_base call left: RSS, S and A against the oracle's three folds
    and, in the fit mode, b' against the oracle's step, bit for bit; nothing but base and the sums is written.  Then the search
    modes on the state a finished joint search left: pass A moves the baseline of every search that is not finished, and the last
    pass on the stacks of the final pass gives p*, b*, rss and the status again."""
    R, T = 70, 300
    y64, sigma = _mixed(R, T, 9)
    y = y64.astype(np.float32)
    g = np.array([GAMMAS[r % 3] for r in range(R)]) if each else GAMMAS[1]
    b = 0.1 * np.cos(np.arange(R))
    dev = _Device(L, y, g, 3)
    dev.given(0.01, 0.4 * sigma, b)
    base, sums = dev.vector(b, True), dev.full(3 * R + GUARD)
    before = dev.ws.clone()
    L.dc_trace_deconv_base_step(dev.d.data_ptr(), dev.f64, dev.ld, R, T, dev.G.data_ptr(), dev.ldG, dev.ws.data_ptr(), dev.n.data_ptr(), br.FIT, None,
                                None, base.data_ptr(), None, None, sums.data_ptr(), dev.stream)
    torch.cuda.synchronize()
    assert dev.ws.cpu().numpy().tobytes() == before.cpu().numpy().tobytes() and (base[R:].cpu().numpy() == CANARY).all()
    flat = sums.cpu().numpy()
    assert (flat[3 * R:] == CANARY).all()                              # three planes of R doubles, dense
    got_sums, got_b = flat[:3 * R].reshape(3, R), base[:R].cpu().numpy()
    for r in range(R):
        G = ref.table(float(g[r]) if each else g, T)
        row = [float(v) for v in y[r]]
        q, S, A = br.sums(row, G, br.forward(row, G, 0.01, 0.4 * sigma[r], float(b[r])), float(b[r]))
        assert (got_sums[0, r], got_sums[1, r], got_sums[2, r]) == (q, S, A), r
        assert got_b[r] == br.step(float(b[r]), S, A, T), r
    assert (got_sums[2] > 0).any() and (got_sums[2] <= T).all()
    # the search modes
    got = dev.search(br.SMIN, sigma, 0.0, 0.0, 7)
    assert set(got['status'].tolist()) == {0, 1, 2}
    p2, b2, r2, s2 = dev.param.clone(), dev.base.clone(), dev.full(R + GUARD), dev.full(R + GUARD, torch.int32)
    L.dc_trace_deconv_base_step(dev.d.data_ptr(), dev.f64, dev.ld, R, T, dev.G.data_ptr(), dev.ldG, dev.ws.data_ptr(), dev.n.data_ptr(), br.PASS_LAST,
                                dev.state.data_ptr(), p2.data_ptr(), b2.data_ptr(), r2.data_ptr(), s2.data_ptr(), None, dev.stream)
    torch.cuda.synchronize()
    again = dict(param=p2[:R].cpu().numpy(), baseline=b2[:R].cpu().numpy(), rss=r2[:R].cpu().numpy(), status=s2[:R].cpu().numpy())
    _same(again, got, ('last pass alone', each), ('param', 'rss', 'status'))
    assert (p2[R:].cpu().numpy() == CANARY).all() and (r2[R:].cpu().numpy() == CANARY).all() and (s2[R:].cpu().numpy() == -7).all()
    b3 = dev.base.clone()
    L.dc_trace_deconv_base_step(dev.d.data_ptr(), dev.f64, dev.ld, R, T, dev.G.data_ptr(), dev.ldG, dev.ws.data_ptr(), dev.n.data_ptr(), br.PASS_A,
                                dev.state.data_ptr(), p2.data_ptr(), b3.data_ptr(), r2.data_ptr(), s2.data_ptr(), None, dev.stream)
    torch.cuda.synchronize()
    done = got['status'] == 1
    assert (b3[:R].cpu().numpy()[done] == dev.state[5 * R:6 * R].cpu().numpy()[done]).all() and (b3[R:].cpu().numpy() == CANARY).all()
    assert ref.same_bits(b3[:R].cpu().numpy(), dev.state[5 * R:6 * R].cpu().numpy())        # plane 5: b, carried


@pytest.mark.parametrize('each', (False, True))
def test_the_plain_sweep_and_the_baseline_sweep_at_zero_fold_the_same_rss(L, each):
    """On the stacks one dc_trace_deconv_ar1_base call left, dc_trace_deconv_base_step at b = 0 and dc_trace_deconv_search_step
    fold the same residual, bit for bit: (y - 0.0) - c is y - c.  The search step gets a state of zeros -- phase START, target 0 --,
    so it records rss_lo = RSS, finishes (RSS >= 0 is never below the target) and, being the last, writes RSS out with status 1
    and p* = 0.  Neither launch writes the workspace or beyond row R."""
    R, T = 70, 300
    y64, sigma = _mixed(R, T, 13)
    y = y64.astype(np.float32)
    g = np.array([GAMMAS[r % 3] for r in range(R)]) if each else GAMMAS[1]
    dev = _Device(L, y, g, 3)
    dev.given(0.01, 0.4 * sigma, 0.0)
    before = dev.ws.clone()
    base, sums = dev.vector(0.0, True), dev.full(3 * R + GUARD)
    L.dc_trace_deconv_base_step(dev.d.data_ptr(), dev.f64, dev.ld, R, T, dev.G.data_ptr(), dev.ldG, dev.ws.data_ptr(), dev.n.data_ptr(), br.FIT, None,
                                None, base.data_ptr(), None, None, sums.data_ptr(), dev.stream)
    state = dev.full(5 * R + GUARD)
    state[:5 * R] = 0.0
    param, rss, status = dev.vector(0.0, True), dev.full(R + GUARD), dev.full(R + GUARD, torch.int32)
    L.dc_trace_deconv_search_step(dev.d.data_ptr(), dev.f64, dev.ld, R, T, dev.G.data_ptr(), dev.ldG, dev.ws.data_ptr(), dev.n.data_ptr(), 1,
                                  state.data_ptr(), param.data_ptr(), rss.data_ptr(), status.data_ptr(), dev.stream)
    dev.check()
    want = sums.cpu().numpy()
    assert rss[:R].cpu().numpy().tobytes() == want[:R].tobytes() and (want[:R] > 0).any()
    assert (status[:R].cpu().numpy() == 1).all() and param[:R].cpu().numpy().tobytes() == np.zeros(R).tobytes()
    assert dev.ws.cpu().numpy().tobytes() == before.cpu().numpy().tobytes()
    for name, a in (('sums', sums[3 * R:]), ('base', base[R:]), ('state', state[5 * R:]), ('param', param[R:]), ('rss', rss[R:])):
        assert (a.cpu().numpy() == CANARY).all(), name
    assert (status[R:].cpu().numpy() == -7).all()


def test_trace_deconvolver_with_a_baseline(L):
    """TraceDeconvolver(baseline=) end to end: 'fit' at fixed parameters and with the search, a given scalar, array and resident
    tensor (read in place, never written), numpy and resident traces; 'baseline' of every object."""
    from deep_calcium_amd import TraceDeconvolver
    from deep_calcium_amd.deconv import trace_noise
    y = np.stack([br.reach_dff(seed, 0.3, 600, 301)[1] for seed in range(70)])
    g, sigma = GAMMAS[1], trace_noise(y)
    d = torch.from_numpy(y).cuda()
    joint = TraceDeconvolver(d, g, constrain='s_min', baseline='fit', rounds=8)
    kinds = ('calcium', 'spikes', 'pools', 'param', 'baseline', 'rss', 'target', 'status')
    want = br.deconvolve_search(y[:6], g, br.SMIN, sigma[:6], 0.0, 0.0, 8)
    _same({k: joint.result(k)[:6] for k in kinds}, want, 'joint', EIGHT)
    _same({k: joint.result(k) for k in kinds}, br.host_search(L, y, g, br.SMIN, sigma, 0.0, 0.0, 8), 'joint, all rows', br.SEARCH_NAMES)
    assert d.cpu().numpy().tobytes() == y.tobytes() and joint.result('baseline').dtype == np.float64 and joint.result_device('baseline').is_cuda
    assert (joint.result('status') == 0).all() and (joint.result('baseline') > 0.5 * sigma).all()
    plain = TraceDeconvolver(d, g, constrain='s_min', rounds=8)
    assert (joint.result('spikes') > 0).sum() < 0.8 * (plain.result('spikes') > 0).sum()      # what it is for: the spurious events go
    g_each = np.array([GAMMAS[r % 3] for r in range(70)])
    for rounds in (1, 5):
        fit = TraceDeconvolver(y, g_each, s_min=2.0 * sigma, lam=0.01, baseline='fit', baseline_rounds=rounds)
        _same({k: fit.result(k) for k in br.FIT_NAMES}, br.host_fit(L, y, g_each, 0.01, 2.0 * sigma, 0.0, rounds), ('fit', rounds), br.FIT_NAMES)
        _same({k: fit.result(k)[:4] for k in br.FIT_NAMES}, br.deconvolve(y[:4], g_each[:4], 0.01, 2.0 * sigma[:4], 0.0, rounds), ('fit, oracle', rounds),
              br.FIT_NAMES)
        with pytest.raises(ValueError, match='is not one of calcium, spikes, pools'):
            fit.result('param')
    b = joint.result('baseline')
    resident = joint.result_device('baseline').clone()
    for given in (b, resident, 0.25):
        dec = TraceDeconvolver(d, g, s_min=joint.result('param'), baseline=given)
        want_b = np.full(70, 0.25) if isinstance(given, float) else b
        assert ref.same_bits(dec.result('baseline'), want_b)
        if not isinstance(given, float):                               # the promise of the joint search: these are its outputs
            for kind in ('calcium', 'spikes', 'pools'):
                assert ref.same_bits(dec.result(kind), joint.result(kind)), kind
    assert ref.same_bits(resident.cpu().numpy(), b)
    with pytest.raises(ValueError, match='baseline must be a contiguous float64 tensor of 70 values'):
        TraceDeconvolver(d, g, baseline=resident[:69])
    with pytest.raises(ValueError, match='baseline must be a contiguous float64 tensor of 70 values'):
        TraceDeconvolver(d, g, baseline=resident.float())


def test_the_defaults_give_the_bits_they_gave(L):
    """Without baseline= the unconstrained and the constrained object call what they called: the bits of the host entry points
    without a baseline, 'baseline' is zeros, and an explicit 0.0 is the default."""
    from deep_calcium_amd import TraceDeconvolver
    from deep_calcium_amd.deconv import trace_noise
    y = np.stack([ref.reach_trace(seed, 0.2, 300)[1] for seed in range(66)])
    sigma = trace_noise(y)
    for kw in ({}, dict(baseline=0.0), dict(baseline=0)):
        dec = TraceDeconvolver(y, GAMMAS[1], s_min=2.0 * sigma, lam=0.05, **kw)
        assert dec.baseline is None
        for kind, b in zip(('calcium', 'spikes', 'pools'), ref.host_entry(L, y, GAMMAS[1], 0.05, 2.0 * sigma)):
            assert ref.same_bits(dec.result(kind), b), kind
        assert dec.result('baseline').tobytes() == np.zeros(66).tobytes()
        con = TraceDeconvolver(y, GAMMAS[1], constrain='s_min', rounds=6, **kw)
        want = sr.host_entry(L, y, GAMMAS[1], sr.SMIN, sigma, 0.0, 6)
        for kind in sr.NAMES:
            assert ref.same_bits(con.result(kind), want[kind]), kind
        assert con.result('baseline').tobytes() == np.zeros(66).tobytes()


def test_deconvolve_traces_device_with_the_baseline_fitted(L, tmp_path):
    """k='noise', baseline='fit' end to end on a small recording (_pair_ref.scene 'two'): dF/F by dff_traces_device, then the
    oracles -- the noise, the estimate, pick_gamma, the joint search -- against the one call, for a given tau, 'auto' and 'each';
    a numeric k with 'fit' and with a constant; without baseline= no new key."""
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
        c, s, info = deconvolve_traces_device(path, rois, window=window, tau=tau, fps=fps, k='noise', lam=0.02, percentile=20, details=True,
                                              baseline='fit')
        want = br.deconvolve_search(dff, g, br.SMIN, sigma, 0.02, 0.0, 24)
        assert ref.same_bits(c, want['calcium']) and ref.same_bits(s, want['spikes']), tau
        assert sorted(info) == ['baseline', 'g', 'g_raw', 'pooled', 'rss', 's_min', 'search_status', 'sigma', 'status']
        assert ref.same_bits(info['s_min'], want['param']) and ref.same_bits(info['rss'], want['rss']), tau
        assert ref.same_bits(info['baseline'], want['baseline']) and ref.same_bits(info['search_status'], want['status']), tau
    c, s, info = deconvolve_traces_device(path, rois, window=window, tau='auto', k=2.0, percentile=20, details=True, baseline='fit')
    want = br.deconvolve(dff, g_pool, 0.0, 2.0 * sigma, 0.0, 8)
    assert ref.same_bits(c, want['calcium']) and ref.same_bits(s, want['spikes']) and ref.same_bits(info['baseline'], want['baseline'])
    c, s, info = deconvolve_traces_device(path, rois, window=window, tau='auto', k=2.0, percentile=20, details=True, baseline=0.05)
    want = br.deconvolve(dff, g_pool, 0.0, 2.0 * sigma, 0.05, 0)
    assert ref.same_bits(c, want['calcium']) and ref.same_bits(s, want['spikes']) and info['baseline'].tolist() == [0.05, 0.05]
    info = deconvolve_traces_device(path, rois, window=window, tau='auto', k=2.0, percentile=20, details=True)[2]
    assert sorted(info) == ['g', 'g_raw', 'pooled', 'sigma', 'status']
