"""Trace dynamics without a GPU: the public names and the ABI, pick_gamma and ar1_tau against their definitions, the oracle's folds
against math.fsum, the library's host entry point against the oracle bit for bit, the structural traces, argument validation in
front of and inside the library, the reach table (what estimating the decay buys over guessing it), and csrc/trace_dyn_math.h
as a stand-alone program under the host sanitizers."""
import ctypes
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _deconv_ref as dref
import _dyn_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (1, 2, 3, 6, 7, 255, 256, 257, 511, 513, 1000)
LAGS = (1, 5, 16)


def test_public_names_and_abi():
    import deep_calcium_amd
    from deep_calcium_amd import _build, _gen_tape, _lib, dynamics
    for name in ('TraceDynamics', 'estimate_ar1_device', 'ar1_tau', 'pick_gamma'):
        assert getattr(deep_calcium_amd, name) is getattr(dynamics, name) and name in deep_calcium_amd.__all__
    assert _lib.header_abi_version() >= 127 and 'trace_dyn.hip' in _build.SOURCES
    assert '-ffp-contract=off' in _build.FILE_FLAGS['trace_dyn.hip']
    protos = _lib.parse_header()
    names = ('dc_trace_noise', 'dc_trace_ar1_estimate', 'dc_ar1_tables', 'dc_trace_deconv_ar1_each', 'dc_trace_ar1_estimate_host')
    assert [len(protos[n][1]) for n in names] == [7, 11, 6, 15, 10]
    assert set(names) <= set(n for n, _ in _gen_tape.prototypes())
    header = open(_lib.HEADER).read()
    assert 'Trace dynamics: noise and AR(1) decay' in header
    assert 'DC_TRACE_DYN_LANES 256' in header and dynamics.LANES == ref.W == 256
    assert 'DC_TRACE_DYN_MAX_LAGS 16' in header and dynamics.MAX_LAGS == 16
    assert 'DC_TRACE_DYN_MAX_GROUPS %d' % dynamics.MAX_GROUPS in header
    assert dynamics.KINDS == ('noise', 'autocov', 'g_raw')
    math_h = open(os.path.join(ROOT, 'deep_calcium_amd', 'csrc', 'trace_dyn_math.h')).read()
    assert '#pragma clang fp contract(off)' in math_h
    for text in (header, open(os.path.join(ROOT, 'deep_calcium_amd', 'deconv.py')).read(), open(os.path.join(ROOT, 'README.md')).read()):
        assert 'estimating g from the autocovariance' not in text and 'estimating `g` from the autocovariance' not in text


def test_dynamics_module_imports_without_torch_or_the_library():
    code = ("import sys, deep_calcium_amd.dynamics as d; "
            "assert 'torch' not in sys.modules and 'deep_calcium_amd._lib' not in sys.modules; print(','.join(d.KINDS))")
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == 'noise,autocov,g_raw', out.stderr[-500:]


# ---- the host helpers ----------------------------------------------------------------------------------------------------------------
def test_pick_gamma_and_ar1_tau_are_their_definitions():
    from deep_calcium_amd import ar1_gamma, ar1_tau, pick_gamma
    nan = float('nan')
    raw = np.array([0.9, 0.01, 1.07, nan, 0.85, 0.998, 0.05, -0.3])
    g_each, status, g_pool = pick_gamma(raw)
    defined = raw[~np.isnan(raw)]
    assert g_pool == float(np.median(defined)) and isinstance(g_pool, float)
    assert g_each.dtype == np.float64 and status.dtype == np.int8
    assert g_each.tolist() == [0.9, 0.05, 0.998, g_pool, 0.85, 0.998, 0.05, 0.05]
    assert status.tolist() == [0, 1, 2, 3, 0, 0, 0, 1]                    # a value ON a bound is fine
    g_each, status, g_pool2 = pick_gamma(raw, g_min=0.5, g_max=0.88, fallback=0.7)
    assert g_pool2 == g_pool and g_each.tolist() == [0.88, 0.5, 0.88, 0.7, 0.85, 0.88, 0.5, 0.5] and status.tolist() == [2, 1, 2, 3, 0, 2, 1, 1]
    # the pooled median is clamped too
    assert pick_gamma([1.2, 1.3, 0.9])[2] == 0.998 and pick_gamma([0.01, 0.02, 0.9])[2] == 0.05
    assert pick_gamma([0.8, 0.9])[2] == float(np.median([0.8, 0.9]))
    # no trace is defined: the fallback serves, and without one it is an error that names trace 0
    g_each, status, g_pool = pick_gamma([nan, nan], fallback=0.9)
    assert g_each.tolist() == [0.9, 0.9] and status.tolist() == [3, 3] and g_pool == 0.9
    with pytest.raises(ValueError, match='trace 0'):
        pick_gamma([nan, nan, nan])
    assert pick_gamma([float('inf'), 0.9])[1].tolist() == [3, 0]          # not finite is undefined
    for kw, what in ((dict(g_min=0.0), r'\(0, 1\)'), (dict(g_max=1.0), r'\(0, 1\)'), (dict(g_min=0.9, g_max=0.8), 'above g_max'),
                     (dict(fallback=1.5), r'\(0, 1\)'), (dict(fallback='x'), r'\(0, 1\)')):
        with pytest.raises(ValueError, match=what):
            pick_gamma([0.9], **kw)
    for bad in (0.9, [], [[0.9]], ['x']):
        with pytest.raises(ValueError, match='g_raw'):
            pick_gamma(bad)
    # ar1_tau: -1 / (fps log g), the inverse of ar1_gamma within one unit in the last place of g -- for g >= 0.5.  The way back
    # is exp(x), x = -1 / (tau fps) = log g, which turns an ABSOLUTE error of x into a RELATIVE error of g: x carries a few
    # roundings of relative size 2^-53, so g is off by about |log g| units of its last place -- below one only while |log g|
    # <= log 2.  Decays of less than 1.5 frames are not what a calcium indicator shows.
    for g in (0.5, 0.7, math.exp(-1.0 / 8), 0.95, 0.998):
        for fps in (1.0, 15.5, 30.0, 1000.0):
            tau = ar1_tau(g, fps)
            assert tau == float(-1.0 / (fps * np.log(g)))
            assert abs(ar1_gamma(tau, fps) - g) <= np.spacing(g)
    assert abs(ar1_tau(math.exp(-1.0 / 8), 16.0) - 0.5) < 1e-15
    for args, what in (((0.0, 30), r'\(0, 1\)'), ((1.0, 30), r'\(0, 1\)'), ((nan, 30), r'\(0, 1\)'), ((0.9, 0), 'fps'), ((0.9, 'x'), 'fps'),
                       ((0.9, float('inf')), 'fps')):
        with pytest.raises(ValueError, match=what):
            ar1_tau(*args)


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
def test_oracle_folds_are_within_the_rounding_bound_of_the_exact_sums():
    """Independent of the order: every q_l the oracle folds against math.fsum of the same rounded terms, within
    (ceil(n / 256) + 9) 2^-53 sum |term| -- the bound of the fold's longest addition path (_dyn_ref.fold_bound)."""
    checked = 0
    for T in (1, 7, 256, 257, 1000, 5000):
        y = ref.traces(6, T, 40 + T, np.float64)
        for r in range(6):
            _, terms = ref.autocov_terms(y[r], 16)
            for q in terms:
                assert abs(ref.fold(q) - math.fsum(q)) <= ref.fold_bound(q), (T, r, len(q))
                checked += 1
    assert checked == 6 * 6 * 17
    assert ref.fold([]) == 0.0 and math.copysign(1.0, ref.fold([])) == 1.0 and ref.fold([-0.0]) == 0.0
    # the order is the lanes, then the tree: terms chosen so that any other order rounds differently
    # lane 0 holds 1 + 2^-53 -> 1 (a tie goes to even) and loses 2^-53 once more at h = 128; the other 254 arrive as sums
    terms = [1.0] + [2.0 ** -53] * 256
    assert ref.fold(terms) == 1.0 + 254 * 2.0 ** -53 and sum(terms) == 1.0


# ---- the host entry point -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', LENGTHS)
def test_host_entry_equals_the_oracle_bit_for_bit(dclib, T):
    for lags in LAGS:
        for dtype, pad in ((np.float32, 0), (np.float64, 0), (np.float32, 3), (np.float64, 5)):
            y = ref.traces(7, T, 31 * T + lags, dtype)
            want = ref.estimate(y, lags)
            got = ref.host_entry(dclib, y, lags, pad=pad)
            for name, a, b in zip(('sigma', 'xc', 'g_raw'), got, want):
                assert ref.same_bits(a, b), (name, T, lags, dtype.__name__, pad)
            if T < lags + 2:
                assert np.isnan(got[2]).all()
            if T < 3:
                assert got[0].tobytes() == np.zeros(7).tobytes()
    # the caller's own noise: it enters A_0 only; sigma is still the trace's, or not computed at all
    y = ref.traces(7, min(T, 300), 9, np.float32)
    sn = np.linspace(0.0, 0.6, 7)
    want = ref.estimate(y, 5, sn=sn)
    got = ref.host_entry(dclib, y, 5, sn=sn)
    assert all(ref.same_bits(a, b) for a, b in zip(got, want))
    got = ref.host_entry(dclib, y, 5, sn=sn, want_sigma=False)
    assert np.isnan(got[0]).all() and ref.same_bits(got[1], want[1]) and ref.same_bits(got[2], want[2])


def test_structural_traces(dclib):
    def both(y, lags=5):
        got, want = ref.host_entry(dclib, y, lags, pad=2), ref.estimate(y, lags)
        assert all(ref.same_bits(a, b) for a, b in zip(got, want)), y.shape
        return got
    # a constant trace (a dyadic value: its sums are exact): no noise, no covariance, no decay
    for T in (7, 300):
        sigma, xc, g = both(np.full((1, T), 1.5, np.float32))
        assert sigma.tobytes() == np.zeros(1).tobytes() and xc.tobytes() == np.zeros(6).tobytes() and np.isnan(g).all()
    # values quantised to 8 levels: the selection meets many ties; both parities of T - 1
    rs = np.random.RandomState(3)
    for T in (100, 101, 256, 257, 1000, 1001):
        y = (rs.randint(0, 8, (3, T)) / 4.0).astype(np.float32)
        sigma, _, _ = both(y)
        assert ref.same_bits(sigma, ref.noise(y)) and (sigma >= 0).all()
    # two levels only: the median of |d - m| is a tie many hundred wide
    y = (rs.rand(2, 400) < 0.5).astype(np.float64)
    both(y)
    # an all-negative trace; a trace that contains -0.0 (and differences that are -0.0)
    both(-5.0 - np.abs(rs.standard_normal((2, 333))))
    z = rs.standard_normal((2, 200)).round(1)
    z[:, ::3] = -0.0
    z[:, 1::3] = 0.0
    assert np.signbit(z).any()
    both(z)
    both(np.where(rs.rand(2, 64) < 0.5, -0.0, 0.0))
    # a noise-free exponential v g^t, long enough to have decayed: close to g from below (the trace is centred on its mean)
    t = np.arange(2000)
    for gtrue in (0.8, math.exp(-1.0 / 8), 0.95):
        _, _, g = both((3.0 * gtrue ** t)[None])
        assert 0.0 < gtrue - g[0] < 0.01, (gtrue, g)
    # adding a constant does not move the estimate (beyond the rounding of the centred values)
    y = ref.traces(1, 2000, 11, np.float64)
    a, b = ref.host_entry(dclib, y, 5), ref.host_entry(dclib, y + 0.75, 5)
    assert abs(a[2][0] - b[2][0]) < 1e-12 and a[0][0] == pytest.approx(b[0][0], rel=1e-12)
    # T == lags + 1 is undefined, T == lags + 2 is defined
    y = ref.traces(1, 7, 12, np.float64)
    assert np.isnan(ref.host_entry(dclib, y[:, :6], 5)[2][0]) and not np.isnan(ref.host_entry(dclib, y, 5)[2][0])


# ---- validation ---------------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    from deep_calcium_amd import _lib
    from deep_calcium_amd.deconv import TraceDeconvolver, deconvolve_traces_device
    from deep_calcium_amd.dynamics import TraceDynamics, estimate_ar1_device

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'lib', boom)
    y = np.arange(12, dtype=np.float32).reshape(2, 6)
    bad = y.copy()
    bad[1, 4] = np.nan
    for args, kw, what in (((y,), dict(lags=0), r'lags must be an integer in \[1, 16\]'),
                           ((y,), dict(lags=17), r'lags must be an integer'),
                           ((y,), dict(lags=5.0), r'lags must be an integer'),
                           ((y,), dict(lags=True), r'lags must be an integer'),
                           ((y,), dict(sn=-0.1), 'sn must be finite and >= 0: trace 0'),
                           ((y,), dict(sn=[0.1, float('nan')]), 'sn must be finite and >= 0: trace 1'),
                           ((y,), dict(sn=[0.1, 0.2, 0.3]), 'sn must be a scalar or one value per trace'),
                           ((y,), dict(sn='x'), 'sn must be a number'),
                           ((bad,), {}, 'row 1 holds a value that is not finite'),
                           ((y.astype(np.int64),), {}, 'float32 or float64'),
                           ((y[0],), {}, 'float32 or float64'),
                           ((y.tolist(),), {}, 'numpy array or a device tensor'),
                           ((y[:, :0],), {}, 'empty'),
                           ((np.broadcast_to(np.float32(0), (1, (1 << 24) + 1)),), {}, r'over the limit of 2\*\*24'),
                           ((np.broadcast_to(np.float32(0), (129, 1 << 24)),), {}, r'over the limit of 2\*\*31')):
        with pytest.raises(ValueError, match=what):
            TraceDynamics(*args, **kw)
        with pytest.raises(ValueError, match=what):
            estimate_ar1_device(*args, **kw)
    with pytest.raises(ValueError, match='above g_max'):
        estimate_ar1_device(y, g_min=0.9, g_max=0.5)
    # a decay per trace
    for g, what in (([0.9, 1.0], r'g must be inside \(0, 1\): trace 1'), ([0.0, 0.9], r'g must be inside \(0, 1\): trace 0'),
                    ([0.9, float('nan')], r'trace 1'), ([0.9], 'one value per trace'), ([[0.9, 0.9]], 'one value per trace'),
                    (['a', 'b'], 'g must be a number or 2 numbers')):
        with pytest.raises(ValueError, match=what):
            TraceDeconvolver(y, g)
    # the one-call front end: refused before the file is even opened
    nowhere = '/nonexistent/dataset.npz'
    ok = [np.array([[1, 2], [3, 4]])]
    for kw, what in ((dict(tau='fast'), "'auto' or 'each'"), (dict(tau='auto', lags=0), 'lags must be an integer'),
                     (dict(tau='each', g_min=0.0), r'\(0, 1\)'), (dict(tau='auto', g_min=0.9, g_max=0.5), 'above g_max'),
                     (dict(tau='auto', fps=0), 'tau and fps'), (dict(tau='each', k=-1), 'k must be finite and >= 0'),
                     (dict(tau='auto', lam=[0.1]), 'lam must be a scalar'), (dict(tau='auto', kind='f'), 'takes dF/F'),
                     (dict(tau=1.0), 'tau and fps'), (dict(tau='auto', details=True, window=4), 'odd')):
        kw.setdefault('window', 3)
        with pytest.raises(ValueError, match=what):
            deconvolve_traces_device(nowhere, ok, **kw)


def test_c_abi_argument_validation_returns_codes(dclib):
    """Refused before any launch (there is no GPU here); the device entry points never follow their pointers."""
    from deep_calcium_amd._lib import DcunetError
    p = 4096                                  # any aligned non-null value
    big = (1 << 24) + 1

    def check(fn, ok, nullable, pointers8, counts):
        """ok: a good argument list with R at index 3 and T at index 4 (traces first)."""
        for i, a in enumerate(ok):
            if i in pointers8 or i == 0:
                if i not in nullable:
                    with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
                        fn(*[None if j == i else b for j, b in enumerate(ok)])
                with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
                    fn(*[(b + (2 if i == 0 else 4)) if j == i else b for j, b in enumerate(ok)])
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            fn(*[(p + 4 if j == 0 else 1 if j == 1 else b) for j, b in enumerate(ok)])            # float64 traces: 8 bytes
        with pytest.raises(DcunetError, match=r'\(-1\).*ld = 7 is below T = 8'):
            fn(*[7 if j == 2 else b for j, b in enumerate(ok)])
        with pytest.raises(DcunetError, match=r'\(-1\).*is_f64 = 2'):
            fn(*[2 if j == 1 else b for j, b in enumerate(ok)])
        for R, T in ((-1, 8), (2, -1)):
            with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
                fn(*[R if j == 3 else T if j == 4 else b for j, b in enumerate(ok)])
        with pytest.raises(DcunetError, match=r'\(-3\).*T = %d is over the limit' % big):
            fn(*[big if j in (2, 4) else 1 if j == 3 else (big + 1 if j == counts.get('ldG') else b) for j, b in enumerate(ok)])
        with pytest.raises(DcunetError, match=r'\(-3\).*R \* T = %d is over the limit' % (129 << 24)):
            fn(*[1 << 24 if j in (2, 4) else 129 if j == 3 else ((1 << 24) + 1 if j == counts.get('ldG') else b) for j, b in enumerate(ok)])
        assert fn(*[0 if j == 3 else b for j, b in enumerate(ok)]) == 0                              # R == 0: no launch
        assert fn(*[0 if j == 4 else b for j, b in enumerate(ok)]) == 0                              # T == 0: no launch

    check(dclib.dc_trace_noise, [p, 0, 8, 2, 8, p, None], (), (5,), {})
    est = [p, 0, 8, 2, 8, 5, p, p, p, p, None]
    check(dclib.dc_trace_ar1_estimate, est, (6, 7), (6, 7, 8, 9), {})
    with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
        dclib.dc_trace_ar1_estimate(*[None if j in (6, 7) else b for j, b in enumerate(est)])      # neither sn nor sigma
    for lags in (0, 17, -1):
        with pytest.raises(DcunetError, match=r'\(-1\).*lags = %d is outside \[1, 16\]' % lags):
            dclib.dc_trace_ar1_estimate(*[lags if j == 5 else b for j, b in enumerate(est)])
    each = [p, 0, 8, 2, 8, p, p, 9, p, p, p, p, p, p, None]
    check(dclib.dc_trace_deconv_ar1_each, each, (), (5, 6, 8, 9, 10, 11, 12), {'ldG': 7})
    with pytest.raises(DcunetError, match=r'\(-1\).*ldG = 8 is below T \+ 1 = 9'):
        dclib.dc_trace_deconv_ar1_each(*[8 if j == 7 else b for j, b in enumerate(each)])
    with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
        dclib.dc_trace_deconv_ar1_each(*[p + 2 if j == 13 else b for j, b in enumerate(each)])      # pools: 4 bytes
    tab = dclib.dc_ar1_tables
    assert tab(p, 0, 8, p, 9, None) == 0
    for args, code, what in (((None, 2, 8, p, 9, None), -1, 'null pointer'), ((p, 2, 8, None, 9, None), -1, 'null pointer'),
                             ((p + 4, 2, 8, p, 9, None), -1, 'misaligned'), ((p, 2, 8, p + 4, 9, None), -1, 'misaligned'),
                             ((p, -1, 8, p, 9, None), -1, 'negative'), ((p, 2, -1, p, 9, None), -1, 'negative'),
                             ((p, 2, 8, p, 8, None), -1, r'ldG = 8 is below T \+ 1 = 9'), ((p, 1, big, p, big + 1, None), -3, 'over the limit'),
                             ((p, 129, 1 << 24, p, (1 << 24) + 1, None), -3, 'over the limit')):
        with pytest.raises(DcunetError, match=r'\(%d\).*%s' % (code, what)):
            tab(*args)

    # the host entry point reads what it is given: real buffers
    host = dclib.dc_trace_ar1_estimate_host
    y = np.zeros((2, 8), np.float32)
    sn, sigma, xc, g = np.zeros(2), np.zeros(2), np.zeros((2, 6)), np.zeros(2)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)               # noqa: E731

    def call(**kw):
        a = dict(y=ptr(y), f64=0, ld=8, R=2, T=8, lags=5, sn=ptr(sn), sigma=ptr(sigma), xc=ptr(xc), g=ptr(g))
        a.update(kw)
        return host(a['y'], a['f64'], a['ld'], a['R'], a['T'], a['lags'], a['sn'], a['sigma'], a['xc'], a['g'])
    assert call() == 0 and call(sn=None) == 0 and call(sigma=None) == 0
    for kw in (dict(y=None), dict(xc=None), dict(g=None), dict(sn=None, sigma=None)):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            call(**kw)
    with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
        call(xc=ctypes.c_void_p(xc.ctypes.data + 4))
    with pytest.raises(DcunetError, match=r'\(-1\).*ld = 7 is below T = 8'):
        call(ld=7)
    for kw in (dict(R=-1), dict(T=-1)):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
            call(**kw)
    for lags in (0, 17):
        with pytest.raises(DcunetError, match=r'\(-1\).*lags = %d' % lags):
            call(lags=lags)
    assert call(R=0) == 0 and call(T=0) == 0


def test_example_refuses_deconvolve_auto_without_dff():
    script = os.path.join(ROOT, 'examples', 'neurons', 'unet2ds_nf.py')
    for extra, what in ((['--deconvolve', 'auto'], '--deconvolve needs --dff'), (['--deconvolve', 'fast', '--dff', '101'], 'expected auto, each or the decay time')):
        r = subprocess.run([sys.executable, script, 'traces', 'nowhere.npz', '-m', 'nowhere.hdf5'] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and what in r.stderr, (extra, r.stderr[-500:])


# ---- reach ---------------------------------------------------------------------------------------------------------------------------
def test_reach_of_the_estimated_decay(capsys):
    """What the estimate buys, on the oracles: 40 seeds of T = 1024, events at rate 0.03 with a true decay of 8 frames
    (g = exp(-1/8) = 0.8825) and amplitude 1 on Gaussian noise, s_min = k sigma_hat, a hit within +-2 frames.  Deconvolved with the
    true g, with decays of half, twice and four times the true tau, with every trace's own estimate (lags 5, clamped) and with
    the pooled median of the 40 estimates.  Measured when the stage was specified -- F1(pooled) below F1(true g) by 0.004 / 0.009,
    above F1(2 tau) by 0.28 / 0.27, above F1(tau / 2) by 0.025 / 0.079, |g_pool - g| 0.0065 / 0.0106, the per-trace estimates at
    sigma 0.2 within 0.042 of the truth."""
    from deep_calcium_amd.dynamics import pick_gamma
    gtrue = math.exp(-1.0 / 8)
    columns = ('true g', 'tau / 2', 'tau x 2', 'tau x 4', 'each', 'pooled')
    rows, pooled, spread = {}, {}, {}
    for sigma, k in ((0.2, 3), (0.3, 2)):
        data = [dref.reach_trace(seed, sigma) for seed in range(40)]
        y = np.stack([d[1] for d in data])
        sig, _, g_raw = ref.estimate(y, 5)
        g_each, status, g_pool = pick_gamma(g_raw)
        assert (status == 0).all()
        pooled[sigma], spread[sigma] = g_pool, (float(g_raw.min()), float(g_raw.max()))
        tot = np.zeros((len(columns), 3), int)                           # hits, true spikes, events
        for i, (sp, trace) in enumerate(data):
            true = np.flatnonzero(sp)
            for c, g in enumerate((gtrue, math.exp(-1.0 / 4), math.exp(-1.0 / 16), math.exp(-1.0 / 32), float(g_each[i]), g_pool)):
                _, s, _ = dref.deconvolve(trace[None], g, 0.0, k * float(sig[i]))
                ev = np.flatnonzero(s[0] > 0)
                tot[c] += (dref.match(true, ev), len(true), len(ev))
        rows[(sigma, k)] = [dref.prf(*t) for t in tot]
    with capsys.disabled():
        print('\n  sigma, k   ' + '   '.join('%-21s' % c for c in columns) + '  (recall / precision / F1)')
        for (sigma, k), row in rows.items():
            print('  %.1f, %d     ' % (sigma, k) + '   '.join('%.3f / %.3f / %.3f' % v for v in row)
                  + '   g_pool %.4f, g_raw %.4f - %.4f' % ((pooled[sigma],) + spread[sigma]))
    for (sigma, k), margin in (((0.2, 3), 0.01), ((0.3, 2), 0.05)):
        f1 = dict(zip(columns, (v[2] for v in rows[(sigma, k)])))
        assert f1['pooled'] >= f1['true g'] - 0.02, (sigma, f1)
        assert f1['pooled'] >= f1['tau x 2'] + 0.2, (sigma, f1)
        assert f1['pooled'] >= f1['tau / 2'] + margin, (sigma, f1)
        assert abs(pooled[sigma] - gtrue) <= 0.02, (sigma, pooled[sigma])
    assert max(abs(v - gtrue) for v in spread[0.2]) <= 0.06, spread[0.2]


# ---- the shared arithmetic ---------------------------------------------------------------------------------------------------------
def test_trace_dyn_math_under_the_host_sanitizers(tmp_path):
    """csrc/trace_dyn_math.h compiled into tests/native/trace_dyn_math_check.cpp with the address and undefined-behaviour sanitizers
    and run as a program of its own: the order key, the medians (nth_element, the kernel's radix descent emulated on the host and
    a full sort agree in value), the fold's order and bound, the autocovariance and the decay against long double."""
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
    exe = str(tmp_path / 'trace_dyn_math_check')
    src = os.path.join(ROOT, 'tests', 'native', 'trace_dyn_math_check.cpp')
    r = subprocess.run([cxx] + flags + [src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'trace_dyn_math_check: ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
