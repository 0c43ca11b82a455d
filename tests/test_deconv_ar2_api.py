"""The AR(2) deconvolution without a GPU: the library's host entry points dc_trace_deconv_ar2_host and
dc_trace_deconv_ar2_constrained_host against the plain-Python oracle (tests/_deconv_ar2_ref.py) in every bit; the pool algebra
against exact rationals; feasibility; the optimality gap against scipy's NNLS; the structural traces; the reach table ("what a rise
time buys"); the front end's refusals; and csrc/deconv_ar2_math.h as a stand-alone program under the host sanitizers."""
import math
import os
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
from scipy import optimize

import _deconv_ar2_ref as a2
import _deconv_ref as ref
import _deconv_search_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAP_BOUND = 0.03                        # the largest gap measured below, 0.0291, rounded up to the next 0.01


def _feasible(y, c, s, what):
    """calcium >= 0 and the spikes above -1e-9 max|y|: what the header promises up to rounding."""
    top = np.abs(np.asarray(y, np.float64)).max()
    assert (c >= 0.0).all() and (s >= -1e-9 * top).all(), (what, c.min(), s.min(), top)


def _mixed(R, T, seed, d, r):
    """Rows in turn: AR(2) events on noise, pure noise, a drifting trace with large values, the ramp, the collapse, the cascade."""
    rs = np.random.RandomState(seed)
    y = np.empty((R, T))
    t = np.arange(T)
    kernel = np.array(a2.table(d, r, T)[0][:T])
    for i in range(R):
        kind = i % 6
        if kind == 0:
            y[i] = np.convolve(rs.poisson(0.05, T) > 0, kernel / kernel.max())[:T] + 0.2 * rs.standard_normal(T)
        elif kind == 1:
            y[i] = 0.5 * rs.standard_normal(T)
        elif kind == 2:
            y[i] = 100.0 * np.cumsum(rs.standard_normal(T)) / np.sqrt(T) + 3.0
        elif kind == 3:
            y[i] = t + 1.0
        elif kind == 4:
            y[i] = -1.0 * t
        else:
            y[i] = np.where(t < T - 1, t + 1.0, -1e6)
    return y


@pytest.mark.parametrize('T', (1, 2, 3, 65))
@pytest.mark.parametrize('roots', a2.ROOTS)
def test_host_entry_points_equal_the_oracle_bit_for_bit(dclib, roots, T):
    """float32 and float64, padded rows and padded table rows whose padding holds NaN, outputs pre-filled with NaN, penalties and a
    given baseline that differ from row to row; both searched parameters."""
    d, r = roots
    R = 13
    seed = 100 * T + int(1000 * d)
    rs = np.random.RandomState(seed)
    y64 = _mixed(R, T, seed, d, r)
    lam = np.where(rs.rand(R) < 0.5, 0.0, 0.3 * rs.rand(R))
    smin = np.where(rs.rand(R) < 0.4, 0.0, 0.8 * rs.rand(R))
    lam[3::6] = smin[3::6] = 0.0
    base = 0.2 * rs.standard_normal(R)
    sigma = np.where(np.arange(R) % 5 == 4, 0.0, 0.1 + 0.4 * rs.rand(R))
    for dtype, pad in ((np.float32, 3), (np.float64, 0)):
        y = y64.astype(dtype)
        for b in (None, base):
            want = a2.deconvolve(y, d, r, lam, smin, b)
            got = a2.host_entry(dclib, y, d, r, lam, smin, b, pad=pad)
            for name, u, v in zip(('calcium', 'spikes', 'pools'), got, want):
                assert ref.same_bits(u, v), (name, roots, T, dtype.__name__, b is not None)
            _feasible(y, got[0], got[1], (roots, T))
            if b is None:
                assert want[2][3] == T and want[2][4] == 1                  # the ramp keeps every pool, the collapse one
        for which, other, rounds in ((sr.SMIN, 0.05, 5), (sr.LAM, 0.1, 24), (sr.SMIN, 0.0, 1)):
            want = a2.constrained(y, d, r, which, sigma, other, rounds)
            got = a2.host_constrained(dclib, y, d, r, which, sigma, other, rounds, pad=pad)
            a2.same(got, want, (roots, T, dtype.__name__, which))
            _feasible(y, got['calcium'], got['spikes'], (roots, T, which))
            assert (got['status'][sigma == 0.0] == 1).all()


def test_table_is_the_definition():
    from deep_calcium_amd import ar2_table
    for d, r in a2.ROOTS:
        for T in (0, 1, 2, 3, 65, 5000):
            H = ar2_table(d, r, T)
            assert H.dtype == np.float64 and H.shape == (3, T + 1) and ref.same_bits(H, np.array(a2.table(d, r, T))), (d, r, T)
    H = ar2_table(0.5, 0.01, 5000)
    assert abs(H[0, -1]) < 2.0 ** -1022 and abs(H[0, 1000]) > 2.0 ** -1022 and np.isfinite(H).all()      # the tail underflows into the subnormals
    for g, rise, what in ((0.9, 0.9, 'rise must be inside'), (0.9, 0.95, 'rise must be inside'), (0.9, 0.0, 'rise must be inside'),
                          (1.0, 0.5, 'g must be inside'), (0.9, float('nan'), 'rise must be inside'), ([0.9, 0.8], 0.5, 'per trace')):
        with pytest.raises(ValueError, match=what):
            ar2_table(g, rise, 8)


def test_pool_algebra_in_exact_rationals():
    """Independent of the pool algorithm's bookkeeping, with the dyadic roots (0.75, 0.25) and T <= 12, in Fractions: the shift
    identity; A and B of every final pool are the direct sums of its frames; v is the exact least-squares value given u.  The float
    oracle makes the same cuts on these inputs and agrees with the rational values to a relative 1e-12.  This validates the oracle
    that the library is held to, not the C++: it runs no library code (the bit-for-bit tests above do)."""
    d, r = 0.75, 0.25
    T = 12
    g1, g2, h = a2.table_exact(d, r, 2 * T)
    for m in range(1, T + 1):
        for k in range(1, T + 1):
            assert h[m + k] == h[m] * h[k] + g2 * h[m - 1] * h[k - 1], (m, k)
    rs = np.random.RandomState(3)
    seen_merge = 0
    for trial in range(60):
        n = 1 + trial % T
        lam = Fraction(int(rs.randint(0, 3)), 8)
        smin = Fraction(int(rs.randint(0, 3)), 16)
        y = [Fraction(int(v), 16) for v in rs.randint(-12, 40, n)]
        if trial % 3 == 0:                     # events with a rise, quantised
            ev = rs.rand(n) < 0.3
            c = np.convolve(ev, [float(v) for v in h[:n]])[:n]
            y = [Fraction(int(round(16 * (a + 0.3 * b))), 16) for a, b in zip(c, rs.standard_normal(n))]
        exact = a2.forward_exact(y, d, r, lam, smin)
        x = [y[t] - (lam * (1 - g1 - g2) if t < n - 2 else (lam * (1 - g1) if t == n - 2 else lam)) for t in range(n)]
        assert sum(p[5] for p in exact) == n
        for p in exact:
            v, u, A, B, t0, l = p
            assert A == sum(h[k] * x[t0 + k] for k in range(l)) and B == sum(h[k - 1] * x[t0 + k] for k in range(1, l)), (trial, t0, l)
            # least squares in v of sum_k (h[k] v + g2 h[k-1] u - x[t0+k])^2, the k = 0 term being (v - x[t0])^2
            num = sum(h[k] * (x[t0 + k] - (g2 * h[k - 1] * u if k >= 1 else 0)) for k in range(l))
            assert v == num / sum(h[k] * h[k] for k in range(l)), (trial, t0, l)
            seen_merge += l > 1
        m = a2.Model(d, r, n)
        pools = a2.forward([float(v) for v in y], m, float(lam), float(smin))
        assert [(p[4], p[5]) for p in pools] == [(p[4], p[5]) for p in exact], trial
        for p, q in zip(pools, exact):
            for i in range(4):
                assert abs(Fraction(p[i]) - q[i]) <= Fraction(1, 10 ** 12) * max(abs(q[i]), 1), (trial, i, p[i], float(q[i]))
    assert seen_merge > 50


def test_optimality_gap_against_nnls(dclib, capsys):
    """NOT promised: optimality.  The greedy pass fits a pool without regard to the pools it later supports.  Against
    scipy.optimize.nnls on the Toeplitz matrix of h (lam = s_min = 0, the reach generator at T = 200, 20 seeds x sigma 0.1 and
    0.3): gap = (RSS_greedy - RSS_nnls) / RSS_nnls is never below -1e-9 -- the greedy solution is feasible for the same problem --
    and at most GAP_BOUND.  Measured: largest 0.0291, smallest 0 to rounding."""
    d, r = a2.REACH_ROOTS
    T = 200
    h = np.array(a2.table(d, r, T)[0][:T])
    K = np.zeros((T, T))
    for k in range(T):
        K[np.arange(k, T), np.arange(T - k)] = h[k]
    gaps = []
    for sigma in (0.1, 0.3):
        for seed in range(20):
            y = a2.reach_trace(seed, sigma, T)[1]
            c, s, _ = a2.host_entry(dclib, y[None], d, r)
            _feasible(y, c, s, (sigma, seed))
            y64 = y.astype(np.float64)
            greedy = float(((y64 - c[0]) ** 2).sum())
            best = float(optimize.nnls(K, y64, maxiter=10 * T)[1]) ** 2
            gaps.append((greedy - best) / best)
    with capsys.disabled():
        print('\n  optimality gap of the greedy AR(2) pass against NNLS, 40 traces: min %.3g, median %.4f, max %.4f' % (min(gaps), np.median(gaps), max(gaps)))
    assert min(gaps) >= -1e-9 and max(gaps) <= GAP_BOUND, (min(gaps), max(gaps))


def test_structural_traces(dclib):
    for d, r in a2.ROOTS:
        for T in (1, 2, 3, 40):
            t = np.arange(T, dtype=np.float64)
            c, s, n = a2.host_entry(dclib, np.stack([t + 1.0, -t]), d, r)
            assert n.tolist() == [T, 1], (d, r, T)
            assert ref.same_bits(c[0], t + 1.0) and is_zero(s[0, :1]) and (s[0, 1:] > 0).all()
            assert is_zero(c[1]) and is_zero(s[1])
            _feasible(np.stack([t + 1.0, -t]), c, s, (d, r, T))


def is_zero(a):
    return a.tobytes() == np.zeros(a.shape).tobytes()                  # +0.0 in every element


# ---- the front end -------------------------------------------------------------------------------------------------------------------
class _Stop(Exception):
    pass


def test_front_end_refusals_before_the_gpu_is_touched(monkeypatch):
    from deep_calcium_amd import TraceDeconvolver, deconvolve_traces_device
    from deep_calcium_amd import deconv
    y = np.zeros((2, 8), np.float32)

    def stop(self, *a, **kw):
        raise _Stop()
    monkeypatch.setattr(TraceDeconvolver, '_open', stop)                # the first thing that touches the library or the GPU
    for kw, what in ((dict(g=0.9, rise=0.9), 'rise must be inside'), (dict(g=0.9, rise=0.95), 'rise must be inside'),
                     (dict(g=0.9, rise=-0.1), 'rise must be inside'), (dict(g=0.9, rise=[0.5, 0.5]), 'rise must be a number'),
                     (dict(g=0.9, rise=0.5, baseline='fit'), 'not built for AR\\(2\\)'),
                     (dict(g=[0.9, 0.8], rise=0.5), 'per trace is not built for AR\\(2\\)'),
                     (dict(g=0.9, rise=0.5, constrain='s_min', baseline=0.1), 'cannot go with constrain')):
        with pytest.raises(ValueError, match=what):
            TraceDeconvolver(y, **kw)
    with pytest.raises(_Stop):                                          # everything else is accepted
        TraceDeconvolver(y, 0.9, rise=0.5, s_min=[0.1, 0.2], lam=0.05, baseline=[0.1, -0.1])
    with pytest.raises(_Stop):
        TraceDeconvolver(y, 0.9, rise=0.5, constrain='lam', sigma=0.1, rounds=3)
    # rise=None runs the existing path: the AR(2) table is not even built
    monkeypatch.setattr(deconv, 'ar2_table', lambda *a: pytest.fail('rise=None built the AR(2) table'))
    with pytest.raises(_Stop):
        TraceDeconvolver(y, 0.9)
    with pytest.raises(_Stop):
        TraceDeconvolver(y, [0.9, 0.8], baseline='fit')
    for kw, what in ((dict(tau='auto', tau_rise=0.1), 'tau_rise needs a number'), (dict(tau='each', tau_rise=0.1, fps=30.0), 'tau_rise needs a number'),
                     (dict(tau=1.0, tau_rise=1.0, fps=30.0), 'rise must be inside'), (dict(tau=1.0, tau_rise=0.1), 'tau and fps'),
                     (dict(tau=1.0, tau_rise=0.1, fps=30.0, baseline='fit'), 'not built for AR\\(2\\)')):
        with pytest.raises(ValueError, match=what):
            deconvolve_traces_device('nowhere.npz', [], 101, **kw)


def test_entry_points_check_the_roots(dclib):
    from deep_calcium_amd._lib import DcunetError
    assert dclib.dc_trace_deconv_ar2_ws_bytes(3, 7) == 40 * 3 * 7 and dclib.dc_trace_deconv_ar2_ws_bytes(0, 7) == 0
    assert dclib.dc_trace_deconv_ar2_ws_bytes(2, (1 << 24) + 1) == 0 and dclib.dc_trace_deconv_ar2_ws_bytes(1 << 20, 1 << 12) == 0
    T = 8
    y = np.zeros((2, T), np.float32)
    H = np.zeros((3, T + 1))
    H[0, :2] = 1.0, 1.0
    v, out, n = np.zeros(2), np.zeros((2, T)), np.zeros(2, np.int32)
    p = a2._ptr
    bad = ((1.0, -0.25), (1.0, -0.5), (1.0, 0.0), (1.0, 0.1), (0.0, -0.1), (-0.5, -0.1), (1.5, -0.4), (float('nan'), -0.1))
    for g1, g2 in bad:                         # equal roots, complex roots, one root, a negative root, a root >= 1, NaN
        with pytest.raises(DcunetError, match=r'\(-1\).*two real roots'):
            dclib.dc_trace_deconv_ar2_host(p(y), 0, T, 2, T, g1, g2, p(H), T + 1, p(v), p(v), None, p(out), p(out), p(n))
        with pytest.raises(DcunetError, match=r'\(-1\).*two real roots'):
            dclib.dc_trace_deconv_ar2_constrained_host(p(y), 0, T, 2, T, g1, g2, p(H), T + 1, 0, p(v), p(v), 3, p(out), p(out), p(n), p(v), p(v), p(n))
        # the device entry points refuse before anything is launched: the pointers are never followed
        with pytest.raises(DcunetError, match=r'\(-1\).*two real roots'):
            dclib.dc_trace_deconv_ar2(64, 0, T, 2, T, g1, g2, 64, T + 1, 64, 64, None, 64, 64, 64, 64, None)
        with pytest.raises(DcunetError, match=r'\(-1\).*two real roots'):
            dclib.dc_trace_deconv_ar2_constrained(64, 0, T, 2, T, g1, g2, 64, T + 1, 0, 64, 64, 3, 64, 64, 64, 64, 64, 64, 64, 64, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*ldH = 8 is below T \+ 1 = 9'):
        dclib.dc_trace_deconv_ar2_host(p(y), 0, T, 2, T, 1.0, -0.1875, p(H), T, p(v), p(v), None, p(out), p(out), p(n))
    with pytest.raises(DcunetError, match=r'\(-1\).*the table does not begin'):
        dclib.dc_trace_deconv_ar2_host(p(y), 0, T, 2, T, 1.25, -0.375, p(H), T + 1, p(v), p(v), None, p(out), p(out), p(n))
    with pytest.raises(DcunetError, match=r'\(-1\).*trace 1: lam'):
        dclib.dc_trace_deconv_ar2_host(p(y), 0, T, 2, T, 1.0, -0.1875, p(H), T + 1, p(np.array([0.0, -1.0])), p(v), None, p(out), p(out), p(n))
    with pytest.raises(DcunetError, match=r'\(-1\).*rounds = 65'):
        dclib.dc_trace_deconv_ar2_constrained_host(p(y), 0, T, 2, T, 1.0, -0.1875, p(H), T + 1, 0, p(v), p(v), 65, p(out), p(out), p(n), p(v), p(v), p(n))
    with pytest.raises(DcunetError, match=r'\(-3\).*over the limit'):
        dclib.dc_trace_deconv_ar2(64, 0, 1 << 25, 2, 1 << 25, 1.0, -0.1875, 64, (1 << 25) + 1, 64, 64, None, 64, 64, 64, 64, None)
    assert dclib.dc_trace_deconv_ar2_host(p(y), 0, T, 0, T, 1.0, -0.1875, p(H), T + 1, p(v), p(v), None, p(out), p(out), p(n)) == 0


def test_example_takes_spike_rise():
    script = os.path.join(ROOT, 'examples', 'neurons', 'unet2ds_nf.py')
    base = [sys.executable, script, 'traces', 'nowhere.npz', '-m', 'nowhere.hdf5', '--dff', '101']
    for extra, what in ((['--spike-rise', '0.1'], '--spike-rise needs --deconvolve TAU'),
                        (['--deconvolve', 'auto', '--spike-rise', '0.1'], '--spike-rise needs --deconvolve TAU'),
                        (['--deconvolve', '1.0', '--fps', '30', '--spike-rise', '0.1', '--spike-baseline', 'fit'], 'not built for AR(2)')):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and what in r.stderr, (extra, r.stderr[-500:])


def test_peak_frame_and_coefficients():
    from deep_calcium_amd.deconv import ar1_gamma, ar2_coefficients, ar2_peak
    d, r = a2.REACH_ROOTS
    assert ar2_coefficients(d, r) == a2.coefficients(d, r)
    h = a2.table(d, r, 50)[0]
    assert ar2_peak(d, r) == int(np.argmax(h)) == 3
    assert ar2_peak(0.5, 0.01) == 0 and ar2_peak(ar1_gamma(1.0, 30.0), ar1_gamma(0.15, 30.0)) == int(np.argmax(a2.table(ar1_gamma(1.0, 30.0), ar1_gamma(0.15, 30.0), 200)[0]))


# ---- what a rise time buys: the reach table --------------------------------------------------------------------------------------
def _totals(truth, spikes):
    tot = np.zeros(3, int)
    for sp, row in zip(truth, spikes):
        true, ev = np.flatnonzero(sp), np.flatnonzero(row > 0)
        tot += (ref.match(true, ev), len(true), len(ev))
    return ref.prf(*tot)


def test_reach_table(dclib, capsys):
    """_deconv_ref.reach_trace's events (Poisson 0.03 a frame, T = 1024) convolved with the AR(2) kernel of the roots (exp(-1/8),
    exp(-1/2)) scaled to peak 1, 40 seeds, s_min = k sigma_hat, a hit within +-2 frames, through the library's host entry points
    (equal to the oracles in every bit by the tests above): AR(1) at g = exp(-1/8) with k in {2, 3}, AR(2) with k in
    {1, 1.5, 2, 3} and AR(2) with s_min searched in 24 rounds.  Asserted: at each sigma the best AR(2) F1 exceeds the best AR(1) F1
    by at least 0.03; the AR(1) precision at sigma 0.1, k = 3 is below 0.6 (every event is found two or three times); the
    searched AR(2) reaches F1 0.85 at sigma 0.1 and 0.2."""
    from deep_calcium_amd.deconv import trace_noise
    d, r = a2.REACH_ROOTS
    assert d == math.exp(-1.0 / 8) and r == math.exp(-1.0 / 2)
    rows = {}
    for sigma in (0.1, 0.2, 0.3):
        made = [a2.reach_trace(seed, sigma) for seed in range(40)]
        truth, y = [m[0] for m in made], np.stack([m[1] for m in made])
        sig = trace_noise(y)
        cells = {}
        for k in (2.0, 3.0):
            cells['AR(1) k = %g' % k] = _totals(truth, ref.host_entry(dclib, y, d, 0.0, k * sig)[1])
        for k in (1.0, 1.5, 2.0, 3.0):
            c, s, _ = a2.host_entry(dclib, y, d, r, 0.0, k * sig)
            _feasible(y, c, s, (sigma, k))
            cells['AR(2) k = %g' % k] = _totals(truth, s)
        found = a2.host_constrained(dclib, y, d, r, sr.SMIN, sig, 0.0, 24)
        _feasible(y, found['calcium'], found['spikes'], (sigma, 'searched'))
        cells['AR(2) searched'] = _totals(truth, found['spikes'])
        rows[sigma] = (cells, np.bincount(found['status'], minlength=3))
    order = list(rows[0.1][0])
    with capsys.disabled():
        print('\n  recall / precision / F1, 40 seeds; the last column: status of the search, bracketed / zero / never bracketed')
        print('  sigma  ' + '  '.join('%-21s' % n for n in order))
        for sigma, (cells, counts) in rows.items():
            print('  %.1f    %s  %d / %d / %d' % (sigma, '  '.join('%.3f / %.3f / %.3f' % cells[n] for n in order), counts[0], counts[1], counts[2]))
    for sigma, (cells, _) in rows.items():
        best1 = max(cells[n][2] for n in order if n.startswith('AR(1)'))
        best2 = max(cells[n][2] for n in order if n.startswith('AR(2) k'))
        assert best2 >= best1 + 0.03, (sigma, best2, best1)
    assert rows[0.1][0]['AR(1) k = 3'][1] < 0.6, rows[0.1][0]['AR(1) k = 3']
    assert rows[0.1][0]['AR(2) searched'][2] >= 0.85 and rows[0.2][0]['AR(2) searched'][2] >= 0.85, (rows[0.1][0], rows[0.2][0])


# ---- the shared arithmetic ---------------------------------------------------------------------------------------------------------
def test_deconv_ar2_math_under_the_host_sanitizers(tmp_path):
    """csrc/deconv_ar2_math.h compiled into tests/native/deconv_ar2_check.cpp with the address and undefined-behaviour sanitizers
    and run as a program of its own: the forward pass on the structural traces (a stack of depth T in T entries), T = 1, and
    random traces of ragged length with buffers and tables exactly as long as they must be."""
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler')
    # sanitizer runtimes linked statically (clang's default; gcc needs the flags): the program is then indifferent to whatever
    # the environment preloads, and the environment is passed through untouched
    flags = ['-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']
    probe = str(tmp_path / 'probe.cpp')
    with open(probe, 'w') as fp:
        fp.write('int main() { return 0; }\n')
    for extra in (['-static-libasan', '-static-libubsan'], []):
        r = subprocess.run([cxx] + flags + extra + [probe, '-o', str(tmp_path / 'probe')], capture_output=True, text=True, timeout=300)
        if r.returncode == 0:
            flags += extra
            break
    else:
        pytest.skip('the host compiler cannot link the sanitizer runtimes: %s' % r.stderr[-300:])
    exe = str(tmp_path / 'deconv_ar2_check')
    src = os.path.join(ROOT, 'tests', 'native', 'deconv_ar2_check.cpp')
    r = subprocess.run([cxx] + flags + [src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'deconv_ar2_check: ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
