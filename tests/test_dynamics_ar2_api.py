"""The AR(2) coefficients of the trace dynamics without a GPU: the public names and the ABI, the library's host entry point
dc_trace_ar2_solve_host against the plain-Python oracle (tests/_dyn_ar2_ref.py) in every bit, the structural inputs, ar2_roots and
pick_roots against their definitions, argument validation in front of and inside the library, the reach table (what estimating
the rise buys over falling back to AR(1)), and dc_dyn_ar2_solve as a stand-alone program under the host sanitizers."""
import ctypes
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _deconv_ar2_ref as a2
import _deconv_ref as dref
import _deconv_search_ref as sr
import _dyn_ar2_ref as ar2
import _dyn_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 3, 6, 7, 12, 257, 1000)
LAGS = (2, 5, 10, 16)


def test_public_names_and_abi():
    import deep_calcium_amd
    from deep_calcium_amd import _gen_tape, _lib, dynamics
    for name in ('TraceDynamicsAR2', 'estimate_ar2_device', 'ar2_roots', 'pick_roots'):
        assert getattr(deep_calcium_amd, name) is getattr(dynamics, name) and name in deep_calcium_amd.__all__
    assert _lib.header_abi_version() >= 132
    protos = _lib.parse_header()
    names = ('dc_trace_ar2_solve', 'dc_trace_ar2_solve_host')
    assert [len(protos[n][1]) for n in names] == [7, 6]
    assert set(names) <= set(n for n, _ in _gen_tape.prototypes())                 # both can be replayed from a tape
    tramp = open(_gen_tape.OUT).read()
    assert '{"dc_trace_ar2_solve", t_dc_trace_ar2_solve, 7, "plllppp"}' in tramp
    assert '{"dc_trace_ar2_solve_host", t_dc_trace_ar2_solve_host, 6, "plllpp"}' in tramp
    # neither takes a row pitch: they read the small dense xc, not the traces
    for n in names:
        assert not set(protos[n][2]) & {'ld', 'ldG', 'ldH', 'frames', 'tc'}, protos[n][2]
    header = open(_lib.HEADER).read()
    assert 'Trace dynamics: AR(2) coefficients' in header
    assert dynamics.KINDS == ('noise', 'autocov', 'g_raw') and dynamics.AR2_KINDS == ('noise', 'autocov', 'g_raw', 'g12_raw')
    # what is built is no longer listed as not built
    readme = open(os.path.join(ROOT, 'README.md')).read()
    texts = [header, readme] + [open(os.path.join(ROOT, 'deep_calcium_amd', f)).read() for f in ('deconv.py', 'dynamics.py')]
    for text in texts:
        for gone in ('estimating r, or (g1, g2)', 'estimating the rise `r`, or `(g1, g2)`', 'Not built: estimating the rise',
                     'Not built: AR(2), refining', 'under AR(2) ("A rise time in the deconvolution" below): estimating the rise'):
            assert gone not in text, gone
    assert 'Estimating the rise' in readme and "tau_rise='auto'" in readme


# ---- the host entry point -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', LENGTHS)
def test_host_entry_equals_the_oracle_bit_for_bit(dclib, T):
    """xc and sigma are the oracle's (what dc_trace_ar1_estimate_host writes, by tests/test_dynamics_api.py); the caller's own
    noise; and the two entry points of the library chained as TraceDynamicsAR2 chains them."""
    for lags in LAGS:
        for dtype in (np.float32, np.float64):
            y = ref.traces(7, T, 17 * T + lags, dtype)
            sigma, xc, _, want = ar2.estimate(y, lags)
            got = ar2.host_entry(dclib, xc, T, lags, sigma)
            assert ref.same_bits(got, want), (T, lags, dtype.__name__, got, want)
            assert np.isnan(got).all() if T < lags + 2 else True
            assert (np.isnan(got[:, 0]) == np.isnan(got[:, 1])).all()              # both or neither
            s2, xc2, _ = ref.host_entry(dclib, y, lags, pad=3)
            assert ref.same_bits(ar2.host_entry(dclib, xc2, T, lags, s2), want)
        sn = np.linspace(0.0, 0.6, 7)
        _, xc, _, want = ar2.estimate(y, lags, sn=sn)
        assert ref.same_bits(ar2.host_entry(dclib, xc, T, lags, sn), want), (T, lags, 'sn')
    if T >= 257:                           # something is defined there: the test is not about NaN alone
        assert np.isfinite(want).any()


def test_structural_inputs(dclib):
    def both(xc, T, lags, sn):
        xc = np.asarray(xc, np.float64)
        sn = np.broadcast_to(np.asarray(sn, np.float64), (xc.shape[0],))
        got, want = ar2.host_entry(dclib, xc, T, lags, sn), ar2.solve_rows(xc, T, lags, sn)
        assert ref.same_bits(got, want), (xc, T, lags, sn, got, want)
        return got
    for lags in LAGS:
        # an all-zero xc: det == 0.0, undefined
        assert np.isnan(both(np.zeros((2, lags + 1)), 1000, lags, 0.0)).all()
        assert (both(np.zeros((2, lags + 1)), 1000, lags, 0.5) == 0.0).all()      # sn alone fills the diagonal: det = sn^8, g = 0 / det
        # a constant trace (a dyadic value: its sums are exact): no covariance at all
        y = np.full((1, 300), 1.5, np.float32)
        sigma, xc, _, want = ar2.estimate(y, lags)
        assert xc.tobytes() == np.zeros((1, lags + 1)).tobytes() and np.isnan(want).all()
        assert np.isnan(both(xc, 300, lags, sigma)).all()
        # sn so large that c0 < 0: legal, whatever the arithmetic gives
        y = ref.traces(6, 400, 5, np.float64)
        _, xc, _ = ref.estimate(y, lags)
        sn = 2.0 * np.sqrt(xc[:, 0]) + 1.0
        assert ((xc[:, 0] - sn * sn) < 0).all()
        both(xc, 400, lags, sn)
        # T == lags + 1 is undefined, T == lags + 2 is defined
        y = ref.traces(1, lags + 2, 12, np.float64)
        s1, x1, _, w1 = ar2.estimate(y[:, :lags + 1], lags)
        s2, x2, _, w2 = ar2.estimate(y, lags)
        assert np.isnan(both(x1, lags + 1, lags, s1)).all() and np.isnan(w1).all()
        assert not np.isnan(both(x2, lags + 2, lags, s2)).any() and not np.isnan(w2).any()
        assert np.isnan(both(x2, lags + 1, lags, s2)).all()                        # T alone decides
    # an exact AR(2) autocovariance gives its coefficients back
    d, r = a2.REACH_ROOTS
    g1, g2 = a2.coefficients(d, r)
    xc = [1.0, g1 / (1.0 - g2)]
    for k in range(2, 11):
        xc.append(g1 * xc[k - 1] + g2 * xc[k - 2])
    got = both([xc], 1000, 10, 0.0)
    assert abs(got[0, 0] - g1) < 1e-9 and abs(got[0, 1] - g2) < 1e-9, got


# ---- the host helpers ----------------------------------------------------------------------------------------------------------------
def test_ar2_roots_is_the_inverse_of_ar2_coefficients():
    from deep_calcium_amd import ar2_roots
    from deep_calcium_amd.deconv import ar2_coefficients
    pairs = list(a2.ROOTS) + [(0.998, 0.05), (0.9, 0.899), (0.3, 0.2)]
    for d, r in pairs:
        got = ar2_roots(*ar2_coefficients(d, r))
        assert abs(got[0] - d) <= 1e-12 and abs(got[1] - r) <= 1e-12, (d, r, got)
        assert got == ar2.roots(*a2.coefficients(d, r))                            # and the oracle's, in every bit
    g1, g2 = np.array([a2.coefficients(d, r) for d, r in pairs]).T
    dd, rr = ar2_roots(g1, g2)
    assert dd.dtype == np.float64 and np.abs(dd - [p[0] for p in pairs]).max() <= 1e-12 and np.abs(rr - [p[1] for p in pairs]).max() <= 1e-12
    # disc <= 0: complex or equal roots are NaN; NaN in, NaN out
    for g1, g2 in ((1.0, -0.25), (1.0, -0.5), (0.0, 0.0), (float('nan'), -0.1), (1.0, float('nan'))):
        d, r = ar2_roots(g1, g2)
        assert math.isnan(d) and math.isnan(r), (g1, g2)
    with pytest.raises(ValueError, match='one shape'):
        ar2_roots([1.0, 1.0], [-0.1])
    with pytest.raises(ValueError, match='must be numbers'):
        ar2_roots('x', 0.1)


def test_pick_roots_is_its_definition():
    from deep_calcium_amd import pick_roots
    from deep_calcium_amd.dynamics import ROOTS_COMPLEX, ROOTS_FINE, ROOTS_NO_RISE, ROOTS_SLOW, ROOTS_UNDEFINED
    assert (ROOTS_FINE, ROOTS_COMPLEX, ROOTS_NO_RISE, ROOTS_SLOW, ROOTS_UNDEFINED) == (0, 1, 2, 3, 4)
    nan = float('nan')
    c = a2.coefficients
    raw = np.array([c(0.9, 0.5),            # 0 fine
                    (1.0, -0.5),            # 1 complex
                    (1.0, -0.25),           # 1 equal roots: disc == 0
                    c(0.9, -0.2),           # 2 r <= 0: AR(1) by this estimate
                    c(1.05, 0.5),           # 3 d >= 1
                    c(0.999, 0.5),          # 3 d > d_max
                    (nan, -0.1),            # 4 undefined
                    (0.5, float('inf')),    # 4 not finite
                    c(0.8, 0.3),            # 0
                    c(0.85, 0.6),           # 0
                    c(1.2, -0.1),           # 3 before 2: d >= 1 and r <= 0
                    c(0.5, 0.0)])           # 2 r == 0
    roots_each, status, pooled = pick_roots(raw)
    assert status.dtype == np.int8 and status.tolist() == [0, 1, 1, 2, 3, 3, 4, 4, 0, 0, 3, 2]
    assert roots_each.dtype == np.float64 and roots_each.shape == (12, 2)
    fine = [ar2.roots(*raw[i]) for i in (0, 8, 9)]
    assert pooled == (float(np.median([f[0] for f in fine])), float(np.median([f[1] for f in fine]))) and all(isinstance(v, float) for v in pooled)
    assert 0.0 < pooled[1] < pooled[0] <= 0.998
    for i in range(12):
        assert tuple(roots_each[i]) == (ar2.roots(*raw[i]) if status[i] == 0 else pooled), i
    # the independent restatement, in every bit -- on this table and on random coefficients
    rs = np.random.RandomState(5)
    rand = np.stack([rs.uniform(-0.5, 2.0, 400), rs.uniform(-1.0, 0.3, 400)], axis=1)
    rand[::37] = nan
    for table, kw in ((raw, {}), (raw, dict(d_max=0.88)), (rand, {}), (rand, dict(d_max=0.9, fallback=(0.9, 0.5)))):
        got, want = pick_roots(table, **kw), ar2.pick_roots(table, **kw)
        assert ref.same_bits(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2], kw
    assert set(pick_roots(rand)[1].tolist()) == {0, 1, 2, 3, 4}
    # a root ON the bound is fine; an even count pools the mean of the two middle ones
    assert pick_roots([c(0.75, 0.25)], d_max=0.75)[1].tolist() == [0]
    assert pick_roots([c(0.75, 0.25), c(0.5, 0.125)], d_max=0.7499)[1].tolist() == [3, 0]
    two = pick_roots([c(0.75, 0.25), c(0.5, 0.125)])
    assert two[2] == ((0.75 + 0.5) / 2.0, (0.25 + 0.125) / 2.0)
    # no trace of status 0: the fallback serves, and without one it is an error that says what to give instead
    roots_each, status, pooled = pick_roots([(nan, nan), (1.0, -0.5)], fallback=(0.9, 0.4))
    assert pooled == (0.9, 0.4) and status.tolist() == [4, 1] and roots_each.tolist() == [[0.9, 0.4], [0.9, 0.4]]
    with pytest.raises(ValueError, match='give tau and tau_rise'):
        pick_roots([(nan, nan), (1.0, -0.5)])
    # with a status-0 trace the fallback is not used
    assert pick_roots([c(0.9, 0.5), (nan, nan)], fallback=(0.5, 0.1))[0].tolist() == [list(ar2.roots(*c(0.9, 0.5)))] * 2
    for kw, what in ((dict(d_max=0.0), r'\(0, 1\)'), (dict(d_max=1.0), r'\(0, 1\)'), (dict(fallback=0.9), 'pair of roots'),
                     (dict(fallback=(0.5, 0.9)), 'rise must be inside'), (dict(fallback=(1.5, 0.9)), r'\(0, 1\)')):
        with pytest.raises(ValueError, match=what):
            pick_roots([c(0.9, 0.5)], **kw)
    for bad in (0.9, [], [0.9, 0.1], [[0.9]], [['x', 'y']], np.zeros((0, 2))):
        with pytest.raises(ValueError, match='g12_raw'):
            pick_roots(bad)


# ---- validation ---------------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    from deep_calcium_amd import _lib
    from deep_calcium_amd.deconv import TraceDeconvolver, deconvolve_traces_device
    from deep_calcium_amd.dynamics import TraceDynamicsAR2, estimate_ar2_device

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'lib', boom)
    y = np.arange(24, dtype=np.float32).reshape(2, 12)
    bad = y.copy()
    bad[1, 4] = np.nan
    for args, kw, what in (((y,), dict(lags=1), r'lags must be an integer in \[2, 16\]'),
                           ((y,), dict(lags=0), r'lags must be an integer in \[2, 16\]'),
                           ((y,), dict(lags=17), r'lags must be an integer'),
                           ((y,), dict(lags=5.0), r'lags must be an integer'),
                           ((y,), dict(lags=True), r'lags must be an integer'),
                           ((y,), dict(sn=-0.1), 'sn must be finite and >= 0: trace 0'),
                           ((y,), dict(sn=[0.1, 0.2, 0.3]), 'sn must be a scalar or one value per trace'),
                           ((bad,), {}, 'row 1 holds a value that is not finite'),
                           ((y.astype(np.int64),), {}, 'float32 or float64'),
                           ((y.tolist(),), {}, 'numpy array or a device tensor'),
                           ((np.broadcast_to(np.float32(0), (1, (1 << 24) + 1)),), {}, r'over the limit of 2\*\*24')):
        with pytest.raises(ValueError, match=what):
            TraceDynamicsAR2(*args, **kw)
        with pytest.raises(ValueError, match=what):
            estimate_ar2_device(*args, **kw)
    for kw, what in ((dict(d_max=1.0), r'\(0, 1\)'), (dict(fallback=(0.5, 0.9)), 'rise must be inside'), (dict(fallback=0.5), 'pair of roots')):
        with pytest.raises(ValueError, match=what):
            estimate_ar2_device(y, **kw)
    from deep_calcium_amd.dynamics import TraceDynamics
    for order in (0, 3, True, 2.5, 'two'):
        with pytest.raises(ValueError, match='order must be 1 or 2'):
            TraceDynamics(y, order=order)
    with pytest.raises(ValueError, match=r'lags must be an integer in \[2, 16\]'):
        TraceDynamics(y, lags=1, order=2)
    # the one-call front end: refused before the file is even opened.  What is new ...
    nowhere = '/nonexistent/dataset.npz'
    ok = [np.array([[1, 2], [3, 4]])]
    for kw, what in ((dict(tau=1.0, fps=30.0, tau_rise='auto'), "tau_rise='auto' estimates both roots"),
                     (dict(tau='each', tau_rise='auto'), "tau_rise='auto' estimates both roots"),
                     (dict(tau='auto', tau_rise='fast'), "tau_rise must be a number of seconds or 'auto'"),
                     (dict(tau=1.0, fps=30.0, tau_rise='fast'), "tau_rise must be a number of seconds or 'auto'"),
                     (dict(tau='auto', tau_rise='auto', baseline='fit'), r"baseline='fit' is not built for AR\(2\)"),
                     (dict(tau='auto', tau_rise='auto', rise_lags=1), r'rise_lags must be an integer in \[2, 16\]'),
                     (dict(tau='auto', tau_rise='auto', rise_lags=17), 'rise_lags must be an integer'),
                     (dict(tau='auto', tau_rise='auto', g_max=1.0), r'\(0, 1\)'),
                     (dict(tau='auto', tau_rise='auto', k=-1), 'k must be finite and >= 0'),
                     (dict(tau='auto', tau_rise='auto', k='loud'), "'noise'"),
                     (dict(tau='auto', tau_rise='auto', fps=0), 'tau and fps'),
                     (dict(tau='auto', tau_rise='auto', kind='f'), 'takes dF/F'),
                     # ... and every AR(2) refusal there was, with its message
                     (dict(tau='auto', tau_rise=0.1), 'tau_rise needs a number of seconds for tau'),
                     (dict(tau='each', tau_rise=0.1, fps=30.0), 'tau_rise needs a number of seconds for tau'),
                     (dict(tau=1.0, tau_rise=1.0, fps=30.0), 'rise must be inside'),
                     (dict(tau=1.0, tau_rise=0.1), 'tau and fps'),
                     (dict(tau=1.0, tau_rise=0.1, fps=30.0, baseline='fit'), r"baseline='fit' is not built for AR\(2\) \(tau_rise=\)")):
        kw.setdefault('window', 3)
        with pytest.raises(ValueError, match=what):
            deconvolve_traces_device(nowhere, ok, **kw)
    y8 = np.zeros((2, 8), np.float32)
    for kw, what in ((dict(g=0.9, rise=0.9), 'rise must be inside'), (dict(g=0.9, rise=[0.5, 0.5]), 'rise must be a number'),
                     (dict(g=0.9, rise=0.5, baseline='fit'), r'not built for AR\(2\)'),
                     (dict(g=[0.9, 0.8], rise=0.5), r'per trace is not built for AR\(2\)')):
        with pytest.raises(ValueError, match=what):
            TraceDeconvolver(y8, **kw)


def test_c_abi_argument_validation_returns_codes(dclib):
    """Refused before any launch (there is no GPU here): the device entry point never follows its pointers."""
    from deep_calcium_amd._lib import DcunetError
    p = 4096                                  # any aligned non-null value
    big = (1 << 24) + 1
    xc, sn, g12 = np.zeros((2, 6)), np.zeros(2), np.zeros((2, 2))
    ptr = lambda a: a.ctypes.data                                      # noqa: E731
    for fn, ok in ((dclib.dc_trace_ar2_solve, [p, 2, 8, 5, p, p, None]), (dclib.dc_trace_ar2_solve_host, [ptr(xc), 2, 8, 5, ptr(sn), ptr(g12)])):
        for i in (0, 4, 5):
            with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
                fn(*[None if j == i else b for j, b in enumerate(ok)])
            with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
                fn(*[b + 4 if j == i else b for j, b in enumerate(ok)])
        for lags in (-1, 0, 1, 17):
            with pytest.raises(DcunetError, match=r'\(-1\).*lags = %d is outside \[2, 16\]' % lags):
                fn(*[lags if j == 3 else b for j, b in enumerate(ok)])
        for R, T in ((-1, 8), (2, -1)):
            with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
                fn(*[R if j == 1 else T if j == 2 else b for j, b in enumerate(ok)])
        with pytest.raises(DcunetError, match=r'\(-3\).*T = %d is over the limit' % big):
            fn(*[1 if j == 1 else big if j == 2 else b for j, b in enumerate(ok)])
        with pytest.raises(DcunetError, match=r'\(-3\).*R \* T = %d is over the limit' % (129 << 24)):
            fn(*[129 if j == 1 else 1 << 24 if j == 2 else b for j, b in enumerate(ok)])
        assert fn(*[0 if j == 1 else b for j, b in enumerate(ok)]) == 0                               # R == 0: no launch
    g12[:] = -7.0
    assert dclib.dc_trace_ar2_solve_host(ptr(xc), 0, 8, 5, ptr(sn), ptr(g12)) == 0 and (g12 == -7.0).all()
    assert dclib.dc_trace_ar2_solve_host(ptr(xc), 2, 0, 5, ptr(sn), ptr(g12)) == 0 and np.isnan(g12).all()          # T == 0: undefined


def test_example_takes_spike_rise_auto():
    script = os.path.join(ROOT, 'examples', 'neurons', 'unet2ds_nf.py')
    base = [sys.executable, script, 'traces', 'nowhere.npz', '-m', 'nowhere.hdf5', '--dff', '101']
    for extra, what in ((['--deconvolve', 'auto', '--spike-rise', '0.1'], '--spike-rise needs --deconvolve TAU'),          # today's error
                        (['--deconvolve', '1.0', '--fps', '30', '--spike-rise', 'auto'], '--spike-rise auto estimates both roots'),
                        (['--deconvolve', 'auto', '--spike-rise', 'auto', '--spike-baseline', 'fit'], 'not built for AR(2)'),
                        (['--deconvolve', 'auto', '--spike-rise', 'fast'], 'expected auto or the rise time')):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and what in r.stderr, (extra, r.stderr[-500:])


# ---- what estimating the rise buys: the reach table ---------------------------------------------------------------------------------
def _f1(truth, spikes):
    tot = np.zeros(3, int)
    for sp, row in zip(truth, spikes):
        true, ev = np.flatnonzero(sp), np.flatnonzero(row > 0)
        tot += (dref.match(true, ev), len(true), len(ev))
    return dref.prf(*tot)


@pytest.fixture(scope='module')
def reach(dclib):
    """_deconv_ar2_ref.reach_trace, seeds 0 .. 39, T = 1024, true roots (exp(-1/8), exp(-1/2)); s_min searched in 24 rounds against
    sigma_hat; a hit within +-2 frames.  The estimates are the plain-Python oracles' (_dyn_ref.estimate at lags 5 for AR(1), what
    tau='auto' runs; _dyn_ar2_ref.estimate at `lags` for AR(2)) and the picks the oracle's own pick_roots; the deconvolutions go
    through the library's host entry points, equal to their oracles in every bit (tests/test_deconv_search_api.py,
    tests/test_deconv_ar2_api.py).  Computed once."""
    from deep_calcium_amd.dynamics import pick_gamma
    d, r = a2.REACH_ROOTS
    table = {}
    for sigma in (0.1, 0.2, 0.3, 0.5):
        made = [a2.reach_trace(seed, sigma) for seed in range(40)]
        truth, y = [m[0] for m in made], np.stack([m[1] for m in made])
        sig, _, g_raw = ref.estimate(y, 5)
        g_pool = pick_gamma(g_raw)[2]
        row = dict(g_pool=g_pool)
        row['AR(1) auto'] = _f1(truth, sr.host_entry(dclib, y, g_pool, sr.SMIN, sig, 0.0, 24)['spikes'])
        row['AR(2) true'] = _f1(truth, a2.host_constrained(dclib, y, d, r, sr.SMIN, sig, 0.0, 24)['spikes'])
        row['AR(2) 2 tau'] = _f1(truth, a2.host_constrained(dclib, y, math.exp(-1.0 / 16), r, sr.SMIN, sig, 0.0, 24)['spikes'])
        for lags in (5, 10):
            s2, _, _, g12 = ar2.estimate(y, lags)
            assert ref.same_bits(s2, sig)
            _, status, pooled = ar2.pick_roots(g12)
            row['AR(2) pooled, lags %d' % lags] = _f1(truth, a2.host_constrained(dclib, y, pooled[0], pooled[1], sr.SMIN, sig, 0.0, 24)['spikes'])
            row['pooled %d' % lags], row['status %d' % lags] = pooled, np.bincount(status, minlength=5)
            if lags == 10:
                each = [ar2.roots(*g) for g, s in zip(g12.tolist(), status) if s == 0]
                row['spread'] = (min(e[1] for e in each), max(e[1] for e in each))
        table[sigma] = row
    return table


def test_reach_of_the_estimated_rise(reach, capsys):
    """The table of README "Estimating the rise", regenerated and printed.  Asserted at sigma 0.1, 0.2 and 0.3: the F1 with the
    pooled estimated roots (lags 10) is at least the F1 with the true roots minus 0.02, at least 0.10 above the F1 with a decay
    time twice too long, at least 0.20 above AR(1) with its own pooled estimate, and at least 20 of the 40 traces have status 0.
    Measured when the stage was built, F1 (pooled d, r; traces of status 0):
        sigma 0.1: AR(1) 0.401, true roots 0.985, pooled 0.982 (0.8801, 0.6475; 30), lags 5 0.982, twice too long 0.759
        sigma 0.2: AR(1) 0.515, true roots 0.958, pooled 0.954 (0.8902, 0.5982; 32), lags 5 0.948, twice too long 0.671
        sigma 0.3: AR(1) 0.632, true roots 0.900, pooled 0.897 (0.9013, 0.4484; 39), lags 5 0.864, twice too long 0.676
        sigma 0.5: AR(1) 0.691, true roots 0.764, pooled 0.759 (0.9111, 0.1423; 16), lags 5 0.687, twice too long 0.672"""
    columns = ('AR(1) auto', 'AR(2) true', 'AR(2) pooled, lags 10', 'AR(2) pooled, lags 5', 'AR(2) 2 tau')
    with capsys.disabled():
        print('\n  recall / precision / F1, 40 seeds, s_min searched; pooled (d, r) at lags 10; status fine / complex / no rise / slow / undefined')
        print('  sigma  ' + '  '.join('%-21s' % c for c in columns))
        for sigma, row in reach.items():
            print('  %.1f    %s  g_pool %.4f  (%.4f, %.4f)  %s  r of the fine traces %.3f - %.3f' % (
                sigma, '  '.join('%.3f / %.3f / %.3f' % row[c] for c in columns), row['g_pool'], row['pooled 10'][0], row['pooled 10'][1],
                ' / '.join(str(n) for n in row['status 10']), row['spread'][0], row['spread'][1]))
    for sigma in (0.1, 0.2, 0.3):
        row = reach[sigma]
        pooled = row['AR(2) pooled, lags 10'][2]
        assert pooled >= row['AR(2) true'][2] - 0.02, (sigma, pooled, row['AR(2) true'])
        assert pooled >= row['AR(2) 2 tau'][2] + 0.10, (sigma, pooled, row['AR(2) 2 tau'])
        assert pooled >= row['AR(1) auto'][2] + 0.20, (sigma, pooled, row['AR(1) auto'])
        assert row['status 10'][0] >= 20, (sigma, row['status 10'])
        d, r = row['pooled 10']
        assert 0.0 < r < d < 1.0


# ---- the shared arithmetic ---------------------------------------------------------------------------------------------------------
def test_trace_dyn_ar2_solve_under_the_host_sanitizers(tmp_path):
    """dc_dyn_ar2_solve of csrc/trace_dyn_math.h compiled into tests/native/trace_dyn_ar2_check.cpp with the address and
    undefined-behaviour sanitizers and run as a program of its own: every xc a heap buffer of exactly lags + 1 doubles, lags 2 ..
    16; the order restated, exact AR(2) autocovariances, long double, the undefined cases."""
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
    exe = str(tmp_path / 'trace_dyn_ar2_check')
    src = os.path.join(ROOT, 'tests', 'native', 'trace_dyn_ar2_check.cpp')
    r = subprocess.run([cxx] + flags + [src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'trace_dyn_ar2_check: ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
