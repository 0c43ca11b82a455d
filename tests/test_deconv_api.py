"""Spikes by deconvolution without a GPU: the public names and the ABI, the oracle against exact rationals, the library's host entry
point against the oracle bit for bit, the structural traces, argument validation in front of and inside the library, extra= of
write_traces_dataset, the reach table, and csrc/deconv_math.h as a stand-alone program under the host sanitizers."""
import math
import os
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import _deconv_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAMMAS = (math.exp(-1.0 / 2), math.exp(-1.0 / 8), math.exp(-1.0 / 30))
PENALTIES = ((0.0, 0.0), (0.3, 0.0), (0.0, 0.6), (0.1, 0.2))             # (lam, s_min)


def test_public_names_and_abi():
    import deep_calcium_amd
    from deep_calcium_amd import _build, _gen_tape, _lib, deconv
    for name in ('TraceDeconvolver', 'deconvolve_traces_device', 'ar1_gamma', 'ar1_table', 'trace_noise'):
        assert getattr(deep_calcium_amd, name) is getattr(deconv, name) and name in deep_calcium_amd.__all__
    assert _lib.header_abi_version() >= 126 and 'deconv.hip' in _build.SOURCES
    assert '-ffp-contract=off' in _build.FILE_FLAGS['deconv.hip']
    protos = _lib.parse_header()
    for name in ('dc_trace_deconv_ws_bytes', 'dc_trace_deconv_ar1', 'dc_trace_deconv_ar1_host'):
        assert name in protos, name
    assert 'dc_trace_deconv_ar1' in set(n for n, _ in _gen_tape.prototypes())
    assert [len(protos[n][1]) for n in ('dc_trace_deconv_ws_bytes', 'dc_trace_deconv_ar1', 'dc_trace_deconv_ar1_host')] == [2, 14, 11]
    header = open(_lib.HEADER).read()
    assert 'DC_TRACE_DECONV_MAX_FRAMES 16777216L' in header and deconv.MAX_FRAMES == 1 << 24
    assert 'DC_TRACE_DECONV_MAX_SAMPLES 2147483648L' in header and deconv.MAX_SAMPLES == 1 << 31
    assert deconv.KINDS == ('calcium', 'spikes', 'pools')
    math_h = open(os.path.join(ROOT, 'deep_calcium_amd', 'csrc', 'deconv_math.h')).read()
    assert '#pragma clang fp contract(off)' in math_h


def test_deconv_module_imports_without_torch_or_the_library():
    code = ("import sys, deep_calcium_amd.deconv as d; "
            "assert 'torch' not in sys.modules and 'deep_calcium_amd._lib' not in sys.modules; print(','.join(d.KINDS))")
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == 'calcium,spikes,pools', out.stderr[-500:]


# ---- the host helpers ----------------------------------------------------------------------------------------------------------------
def test_host_helpers_are_their_definitions():
    from deep_calcium_amd.deconv import ar1_gamma, ar1_table, trace_noise
    assert ar1_gamma(1.0, 30.0) == float(np.exp(-1.0 / 30.0)) and ar1_gamma(tau=0.5, fps=16) == float(np.exp(-1.0 / 8.0))
    for g in GAMMAS:
        for T in (0, 1, 2, 17, 1000):
            G = ar1_table(g, T)
            assert G.dtype == np.float64 and G.shape == (T + 1,) and G.tolist() == ref.table(g, T)        # the loop, not pow
    assert ar1_table(GAMMAS[2], 1000)[1000] != GAMMAS[2] ** 1000 or ar1_table(GAMMAS[1], 1000)[1000] != GAMMAS[1] ** 1000
    rs = np.random.RandomState(5)
    y = rs.standard_normal((4, 300)).astype(np.float32) * np.array([[0.1], [0.5], [1.0], [2.0]], np.float32)
    got = trace_noise(y)
    assert got.dtype == np.float64 and got.shape == (4,)
    for r in range(4):
        d = np.diff(y[r].astype(np.float64))
        assert got[r] == 1.4826 * np.median(np.abs(d - np.median(d))) / np.sqrt(2.0)
    assert np.allclose(got, [0.1, 0.5, 1.0, 2.0], rtol=0.2)                   # it estimates the sigma of white noise
    assert trace_noise(np.ones((3, 2), np.float32)).tolist() == [0.0, 0.0, 0.0] and trace_noise(np.ones((2, 1))).tolist() == [0.0, 0.0]
    for bad in ((0, 30), (1, 0), (-1, 30), (float('nan'), 30), (1, float('inf')), ('x', 30)):
        with pytest.raises(ValueError, match='tau and fps'):
            ar1_gamma(*bad)
    for bad in (0.0, 1.0, -0.5, 1.5, float('nan')):
        with pytest.raises(ValueError, match=r'\(0, 1\)'):
            ar1_table(bad, 8)
    with pytest.raises(ValueError, match='non-negative integer'):
        ar1_table(0.5, -1)
    with pytest.raises(ValueError, match='numeric'):
        trace_noise(np.ones(5))


# ---- the oracle against exact rationals ------------------------------------------------------------------------------------------
def test_oracle_is_the_exact_rational_solution_on_tiny_dyadic_traces():
    """g = 1/2 and inputs in 1/8ths: every power of g, every weight and every product of them is exact in a double, so the only
    roundings of the oracle are its divisions.  (1) The pool algorithm in Fractions equals the minimiser found by enumerating all
    2^(T-1) cuts -- the algorithm solves the problem it claims to.  (2) The float oracle has the same pools; a pool of at most two
    frames went through at most one division and is the rational value rounded, exactly; a longer one went through at most
    T - 1 <= 5 divisions, each within half an ulp, and multiplications by exact weights that carry them on: 2^-50 relative."""
    rs = np.random.RandomState(17)
    g = Fraction(1, 2)
    seen_long = seen_pools = 0
    for case in range(400):
        T = 1 + case % 6
        y = [Fraction(int(v), 8) for v in rs.randint(-16, 33, size=T)]
        lam = Fraction(int(rs.randint(0, 3)), 4)
        exact = ref.forward_exact(y, g, lam)
        c_exact = [p[0] * g ** k for p in exact for k in range(p[3])]
        assert c_exact == ref.solve_exact(y, g, lam), (case, y, lam)
        got = ref.forward([float(v) for v in y], ref.table(0.5, T), float(lam), 0.0)
        assert [(p[2], p[3]) for p in got] == [(p[2], p[3]) for p in exact], (case, y, lam)
        for p, q in zip(got, exact):
            want = float(q[0])                                # Fraction -> float rounds to nearest
            if p[3] <= 2:
                assert p[0] == want and p[1] == float(q[1]), (case, y, lam)
            else:
                assert abs(p[0] - want) <= 2.0 ** -50 * abs(want) and p[1] == float(q[1]), (case, y, lam)
                seen_long += 1
        seen_pools += len(got)
    assert seen_long > 50 and seen_pools > 400


# ---- the host entry point -----------------------------------------------------------------------------------------------------------
def _cases(T, seed):
    """Three rows: events on noise, pure noise around zero, a drifting trace with large values."""
    rs = np.random.RandomState(seed)
    sp = rs.poisson(0.05, T) > 0
    a = np.convolve(sp, np.exp(-np.arange(T) / 8.0))[:T] + 0.2 * rs.standard_normal(T)
    b = 0.5 * rs.standard_normal(T)
    c = 100.0 * np.cumsum(rs.standard_normal(T)) / np.sqrt(T) + 3.0
    return np.stack([a, b, c])


@pytest.mark.parametrize('T', (1, 2, 3, 17, 256, 1000))
def test_host_entry_equals_the_oracle_bit_for_bit(dclib, T):
    for gi, g in enumerate(GAMMAS):
        for pi, (lam, smin) in enumerate(PENALTIES):
            for dtype, pad in ((np.float32, 0), (np.float64, 0), (np.float32, 3), (np.float64, 5)):
                y = _cases(T, 100 * gi + 10 * pi + T).astype(dtype)
                want = ref.deconvolve(y, g, lam, smin)
                got = ref.host_entry(dclib, y, g, lam, smin, pad=pad)
                for name, a, b in zip(('calcium', 'spikes', 'pools'), got, want):
                    assert ref.same_bits(a, b), (name, T, g, lam, smin, dtype.__name__, pad)
                assert not np.signbit(got[0]).any() and (got[1][:, 0] == 0).all() and (got[2] >= 1).all() and (got[2] <= T).all()
    # per-trace penalties that differ from row to row
    y = _cases(min(T, 300), 7).astype(np.float32)
    lam, smin = np.array([0.0, 0.2, 0.05]), np.array([0.3, 0.0, 10.0])
    got, want = ref.host_entry(dclib, y, GAMMAS[1], lam, smin), ref.deconvolve(y, GAMMAS[1], lam, smin)
    assert all(ref.same_bits(a, b) for a, b in zip(got, want))


def test_structural_traces(dclib):
    g = GAMMAS[2]
    T = 200
    zero = np.zeros(T).tobytes()                                                    # +0.0 in every bit
    # the ramp: no merge, the stack reaches depth T
    ramp = np.arange(1, T + 1, dtype=np.float64)[None]
    c, s, n = ref.host_entry(dclib, ramp, g)
    assert n.tolist() == [T] and np.array_equal(c, ramp) and s[0, 0] == 0 and (s[0, 1:] > 0).all()
    assert all(ref.same_bits(a, b) for a, b in zip((c, s, n), ref.deconvolve(ramp, g)))
    # the collapse: one pool of length T whose value is negative: calcium and spikes +0.0 everywhere
    fall = -np.arange(T, dtype=np.float64)[None]
    c, s, n = ref.host_entry(dclib, fall, g)
    assert n.tolist() == [1] and c.tobytes() == zero and s.tobytes() == zero
    # the cascade: the last frame merges its way down through every pool of the ramp
    casc = np.concatenate([ramp[0], [-1e6]])[None]
    c, s, n = ref.host_entry(dclib, casc, g)
    assert n.tolist() == [1] and c.tobytes() == np.zeros(T + 1).tobytes() and s.tobytes() == np.zeros(T + 1).tobytes()
    assert ref.deconvolve(casc, g)[2].tolist() == [1] and ref.deconvolve(casc[:, :T], g)[2].tolist() == [T]
    for gg in GAMMAS[:2]:                                                           # faster decays: the cascade stops part way
        got, want = ref.host_entry(dclib, casc, gg), ref.deconvolve(casc, gg)
        assert all(ref.same_bits(a, b) for a, b in zip(got, want)) and 1 < got[2][0] < T
    # a constant trace: c = g c + s with a constant s > 0 is feasible, so nothing merges without a threshold; with s_min above
    # the steady spike 1.5 (1 - g) frames merge until the pool has decayed by more than s_min
    const = np.full((1, T), 1.5, np.float32)
    for lam, smin, pools in ((0.0, 0.0, T), (0.2, 0.0, None), (0.0, 0.5, None)):
        got, want = ref.host_entry(dclib, const, g, lam, smin), ref.deconvolve(const, g, lam, smin)
        assert all(ref.same_bits(a, b) for a, b in zip(got, want))
        assert got[2].tolist() == [pools] if pools is not None else 1 < got[2][0] < T or smin == 0.0
    # one frame: one pool, mu = lam, no spike
    for v, lam, want_c in ((2.0, 0.0, 2.0), (2.0, 0.5, 1.5), (-1.0, 0.0, 0.0), (0.25, 0.5, 0.0)):
        c, s, n = ref.host_entry(dclib, np.array([[v]], np.float32), g, lam, 0.3)
        assert n.tolist() == [1] and c.tobytes() == np.array([[want_c]]).tobytes() and s.tobytes() == np.zeros(1).tobytes()


# ---- validation ---------------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    from deep_calcium_amd import _lib
    from deep_calcium_amd.deconv import TraceDeconvolver, deconvolve_traces_device

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'lib', boom)
    y = np.arange(12, dtype=np.float32).reshape(2, 6)
    bad = y.copy()
    bad[1, 4] = np.nan
    inf = y.astype(np.float64)
    inf[0, 0] = -np.inf
    for args, kw, what in (((y, 0.0), {}, r'\(0, 1\)'),
                           ((y, 1.0), {}, r'\(0, 1\)'),
                           ((y, -0.1), {}, r'\(0, 1\)'),
                           ((y, float('nan')), {}, r'\(0, 1\)'),
                           ((y, 'fast'), {}, r'\(0, 1\)'),
                           ((y, 0.9), dict(lam=-0.1), 'lam must be finite and >= 0: trace 0'),
                           ((y, 0.9), dict(lam=[0.0, float('nan')]), 'lam must be finite and >= 0: trace 1'),
                           ((y, 0.9), dict(s_min=[0.1, -1.0]), 's_min must be finite and >= 0: trace 1'),
                           ((y, 0.9), dict(s_min=float('inf')), 's_min must be finite'),
                           ((y, 0.9), dict(s_min=[0.1, 0.2, 0.3]), 's_min must be a scalar or one value per trace'),
                           ((y, 0.9), dict(lam=np.zeros((2, 1))), 'lam must be a scalar or one value per trace'),
                           ((y, 0.9), dict(lam='x'), 'lam must be a number'),
                           ((bad, 0.9), {}, 'row 1 holds a value that is not finite'),
                           ((inf, 0.9), {}, 'row 0 holds a value that is not finite'),
                           ((y.astype(np.int64), 0.9), {}, 'float32 or float64'),
                           ((y.astype(np.float16), 0.9), {}, 'float32 or float64'),
                           ((y[0], 0.9), {}, 'float32 or float64'),
                           ((y.tolist(), 0.9), {}, 'numpy array or a device tensor'),
                           ((y[:, :0], 0.9), {}, 'empty'),
                           ((y[:0], 0.9), {}, 'empty'),
                           ((np.broadcast_to(np.float32(0), (1, (1 << 24) + 1)), 0.9), {}, r'over the limit of 2\*\*24'),
                           ((np.broadcast_to(np.float32(0), (129, 1 << 24)), 0.9), {}, r'over the limit of 2\*\*31')):
        with pytest.raises(ValueError, match=what):
            TraceDeconvolver(*args, **kw)
    # the one-call front end: refused before the file is even opened
    nowhere = '/nonexistent/dataset.npz'
    ok = [np.array([[1, 2], [3, 4]])]
    for kw, what in ((dict(window=3, tau=0.0, fps=30), 'tau and fps'), (dict(window=3, tau=1.0, fps=-1), 'tau and fps'),
                     (dict(window=3, tau=1.0, fps=30, k=-1), 'k must be finite and >= 0'), (dict(window=3, tau=1.0, fps=30, k='x'), 'k must be a number'),
                     (dict(window=3, tau=1.0, fps=30, lam=-1.0), 'lam must be finite'), (dict(window=3, tau=1.0, fps=30, lam=[0.1]), 'lam must be a scalar'),
                     (dict(window=3, tau=1.0, fps=30, kind='f'), 'takes dF/F'), (dict(window=4, tau=1.0, fps=30), 'odd'),
                     (dict(window=3, tau=1.0, fps=30, percentile=101), r'\[0, 100\]')):
        with pytest.raises(ValueError, match=what):
            deconvolve_traces_device(nowhere, ok, **kw)


def test_c_abi_argument_validation_returns_codes(dclib):
    """Refused before any launch (there is no GPU here); the device entry point never follows its pointers."""
    from deep_calcium_amd._lib import DcunetError
    p = 4096                                  # any aligned non-null value
    dev, ws = dclib.dc_trace_deconv_ar1, dclib.dc_trace_deconv_ws_bytes
    ok = [p, 0, 8, 2, 8, 0.9, p, p, p, p, p, p, p, None]
    for i in (0, 6, 7, 8, 9, 10, 11, 12):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            dev(*[None if j == i else a for j, a in enumerate(ok)])
    for i in (6, 7, 8, 9, 10, 11):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            dev(*[a + 4 if j == i else a for j, a in enumerate(ok)])
    for i in (0, 12):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            dev(*[a + 2 if j == i else a for j, a in enumerate(ok)])
    with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
        dev(*[(p + 4 if j == 0 else 1 if j == 1 else a) for j, a in enumerate(ok)])       # float64 traces: 8 bytes
    assert dev(*[(0 if j == 3 else p + 4 if j == 0 else a) for j, a in enumerate(ok)]) == 0      # float32 traces: 4 bytes (R = 0: no launch)
    with pytest.raises(DcunetError, match=r'\(-1\).*ld = 7 is below T = 8'):
        dev(*[7 if j == 2 else a for j, a in enumerate(ok)])
    for R, T in ((-1, 8), (2, -1)):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
            dev(p, 0, 8, R, T, 0.9, p, p, p, p, p, p, p, None)
    with pytest.raises(DcunetError, match=r'\(-1\).*is_f64 = 2'):
        dev(*[2 if j == 1 else a for j, a in enumerate(ok)])
    for g in (0.0, 1.0, -0.5, 1.5, float('nan')):
        with pytest.raises(DcunetError, match=r'\(-1\).*outside \(0, 1\)'):
            dev(*[g if j == 5 else a for j, a in enumerate(ok)])
    big = (1 << 24) + 1
    with pytest.raises(DcunetError, match=r'\(-3\).*T = %d is over the limit' % big):
        dev(p, 0, big, 1, big, 0.9, p, p, p, p, p, p, p, None)
    with pytest.raises(DcunetError, match=r'\(-3\).*R \* T = %d is over the limit' % (129 << 24)):
        dev(p, 0, 1 << 24, 129, 1 << 24, 0.9, p, p, p, p, p, p, p, None)
    assert dev(p, 0, 8, 0, 8, 0.9, p, p, p, p, p, p, p, None) == 0 and dev(p, 0, 8, 2, 0, 0.9, p, p, p, p, p, p, p, None) == 0
    assert ws(2, 8) == 24 * 2 * 8 and ws(128, 1 << 24) == 24 << 31 and ws(65, 257) == 24 * 65 * 257
    assert ws(0, 8) == 0 and ws(2, 0) == 0 and ws(-1, 8) == 0 and ws(1, big) == 0 and ws(129, 1 << 24) == 0

    # the host entry point reads what it is given: real buffers
    import ctypes
    host = dclib.dc_trace_deconv_ar1_host
    y = np.zeros((2, 8), np.float32)
    G = np.cumprod(np.concatenate([[1.0], np.full(8, 0.9)]))
    lam, smin = np.zeros(2), np.zeros(2)
    c, s, n = np.zeros((2, 8)), np.zeros((2, 8)), np.zeros(2, np.int32)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)               # noqa: E731

    def call(**kw):
        a = dict(y=ptr(y), f64=0, ld=8, R=2, T=8, G=ptr(G), lam=ptr(lam), smin=ptr(smin), c=ptr(c), s=ptr(s), n=ptr(n))
        a.update(kw)
        return host(a['y'], a['f64'], a['ld'], a['R'], a['T'], a['G'], a['lam'], a['smin'], a['c'], a['s'], a['n'])
    assert call() == 0
    for name in ('y', 'G', 'lam', 'smin', 'c', 's', 'n'):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            call(**{name: None})
    with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
        call(G=ctypes.c_void_p(G.ctypes.data + 4))
    with pytest.raises(DcunetError, match=r'\(-1\).*ld = 7 is below T = 8'):
        call(ld=7)
    for kw in (dict(R=-1), dict(T=-1, ld=8)):
        with pytest.raises(DcunetError, match=r'\(-1\).*negative'):
            call(**kw)
    for g in (0.0, 1.0, -0.5, 1.5, float('nan')):
        Gb = np.array([1.0, g] + [0.0] * 7)
        with pytest.raises(DcunetError, match=r'\(-1\).*outside \(0, 1\)'):
            call(G=ptr(Gb))
    with pytest.raises(DcunetError, match=r'\(-1\).*G\[0\]'):
        call(G=ptr(np.full(9, 0.9)))
    for what, vals in (('lam', [0.0, -0.1]), ('smin', [float('nan'), 0.0]), ('smin', [0.0, -1.0])):
        with pytest.raises(DcunetError, match=r'\(-1\).*trace %d.*negative' % (0 if what == 'smin' and vals[0] != 0.0 else 1)):
            call(**{what: ptr(np.array(vals))})
    assert call(R=0) == 0 and call(T=0) == 0


# ---- extra= of write_traces_dataset ----------------------------------------------------------------------------------------------------
def test_extra_datasets_leave_the_file_without_them_unchanged(tmp_path):
    from deep_calcium_amd import hdf5_min
    from deep_calcium_amd.traces import write_traces_dataset
    import inspect
    assert list(inspect.signature(write_traces_dataset).parameters) == ['path', 'traces', 'name', 'spikes', 'extra']
    rs = np.random.RandomState(2)
    tr = rs.standard_normal((3, 20)).astype(np.float32)
    sp = rs.rand(3, 20) < 0.1

    def as_before(path, traces, name, spikes=None):
        """The writer as it was before the argument existed."""
        w = hdf5_min.Writer()
        w.attrs['name'] = str(name)
        w.create_dataset('traces', data=traces)
        if spikes is not None:
            w.create_dataset('spikes', data=np.asarray(spikes).astype(np.uint8))
        w.save(path)
    for i, spikes in enumerate((None, sp)):
        a, b, c, d = [str(tmp_path / ('%s%d.hdf5' % (x, i))) for x in 'abcd']
        as_before(a, tr, 'nf.00', spikes)
        write_traces_dataset(b, tr, 'nf.00', spikes)
        write_traces_dataset(c, tr, 'nf.00', spikes, extra=None)
        write_traces_dataset(d, tr, 'nf.00', spikes, extra={})
        assert open(a, 'rb').read() == open(b, 'rb').read() == open(c, 'rb').read() == open(d, 'rb').read()
    cal, dec = rs.rand(3, 20), rs.rand(3, 20)
    path = write_traces_dataset(str(tmp_path / 'e.hdf5'), tr, 'nf.00', extra=dict(calcium=cal, deconvolved=dec))
    f = hdf5_min.File(path)
    assert np.array_equal(np.asarray(f['traces']), tr) and f['calcium'].dtype == np.float64
    assert np.array_equal(np.asarray(f['calcium']), cal) and np.array_equal(np.asarray(f['deconvolved']), dec)
    path = write_traces_dataset(str(tmp_path / 'e.npz'), tr, 'nf.00', sp, extra=dict(calcium=cal))
    z = np.load(path)
    assert sorted(z.files) == ['calcium', 'name', 'spikes', 'traces'] and np.array_equal(z['calcium'], cal)
    for extra, what in ((dict(calcium=cal[:, :5]), 'extra'), (dict(traces=cal), 'cannot name'), ({'a/b': cal}, 'cannot name'), ({3: cal}, 'cannot name'),
                        (dict(calcium=cal.astype(str)), 'extra')):
        with pytest.raises(ValueError, match=what):
            write_traces_dataset(str(tmp_path / 'bad.hdf5'), tr, 'nf.00', extra=extra)


def test_example_refuses_deconvolve_without_dff_or_fps():
    script = os.path.join(ROOT, 'examples', 'neurons', 'unet2ds_nf.py')
    for extra, what in ((['--deconvolve', '1.0', '--fps', '30'], '--deconvolve needs --dff'), (['--deconvolve', '1.0', '--dff', '101'], '--deconvolve needs --fps')):
        r = subprocess.run([sys.executable, script, 'traces', 'nowhere.npz', '-m', 'nowhere.hdf5'] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and what in r.stderr, (extra, r.stderr[-500:])


# ---- reach ---------------------------------------------------------------------------------------------------------------------------
def test_reach_against_the_thresholded_first_difference(capsys):
    """What the stage buys, on the oracle: 40 seeds of T = 1024, events at rate 0.03 with a decay of 8 frames and amplitude 1 on
    Gaussian noise, s_min = k sigma_hat, a hit within +-2 frames; the comparator thresholds the first difference at
    k sqrt(2) sigma_hat.  Measured when the stage was specified: F1 0.995 against 0.760 at sigma 0.2, k 3, and 0.972 against
    0.581 at sigma 0.3, k 2; the asserted margins are several times the seed-to-seed scatter."""
    from deep_calcium_amd.deconv import trace_noise
    g = math.exp(-1.0 / 8)
    rows = {}
    for sigma, k in ((0.1, 3), (0.2, 3), (0.3, 2), (0.3, 3), (0.5, 2)):
        tot = np.zeros((2, 3), int)                                      # hits, true spikes, events: deconvolution / first difference
        for seed in range(40):
            sp, y = ref.reach_trace(seed, sigma)
            sig = float(trace_noise(y[None])[0])
            _, s, _ = ref.deconvolve(y[None], g, 0.0, k * sig)
            true = np.flatnonzero(sp)
            ev = np.flatnonzero(s[0] > 0)
            fd = np.flatnonzero(np.diff(y.astype(np.float64)) > k * np.sqrt(2.0) * sig) + 1
            tot[0] += (ref.match(true, ev), len(true), len(ev))
            tot[1] += (ref.match(true, fd), len(true), len(fd))
        rows[(sigma, k)] = [ref.prf(*t) for t in tot]
    with capsys.disabled():
        print('\n  sigma  k   deconvolution (recall / precision / F1)   thresholded first difference')
        for (sigma, k), (a, b) in rows.items():
            print('  %.1f    %d   %.3f / %.3f / %.3f                      %.3f / %.3f / %.3f' % ((sigma, k) + a + b))
    assert rows[(0.2, 3)][0][2] >= 0.98 and rows[(0.2, 3)][1][2] <= 0.80
    assert rows[(0.3, 2)][0][2] >= 0.95 and rows[(0.3, 2)][1][2] <= 0.65


# ---- the shared arithmetic ---------------------------------------------------------------------------------------------------------
def test_deconv_math_under_the_host_sanitizers(tmp_path):
    """csrc/deconv_math.h compiled into tests/native/deconv_math_check.cpp with the address and undefined-behaviour sanitizers and
    run as a program of its own: every merge and whole traces against a long double restatement within 1e-12 relative, and the
    stack the step is given checks its bounds."""
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
    exe = str(tmp_path / 'deconv_math_check')
    src = os.path.join(ROOT, 'tests', 'native', 'deconv_math_check.cpp')
    r = subprocess.run([cxx] + flags + [src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'deconv_math_check: ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
