"""The noise-constrained search without a GPU: the public names and the ABI, the library's host entry point against the plain-Python
oracle (tests/_deconv_search_ref.py) bit for bit, the three statuses constructed, the invariants on the reach traces, argument
validation in front of the library, the reach table, and csrc/deconv_search_math.h as a stand-alone program under the host
sanitizers."""
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _deconv_ref as ref
import _deconv_search_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G8 = math.exp(-1.0 / 8)


def test_public_names_and_abi():
    from deep_calcium_amd import _gen_tape, _lib, deconv
    assert _lib.header_abi_version() >= 128
    protos = _lib.parse_header()
    names = ('dc_trace_deconv_search_state_bytes', 'dc_trace_deconv_ar1_constrained', 'dc_trace_deconv_ar1_constrained_host')
    assert [len(protos[n][1]) for n in names] == [1, 22, 16]
    assert 'dc_trace_deconv_ar1_constrained' in set(n for n, _ in _gen_tape.prototypes())
    header = open(_lib.HEADER).read()
    for text in ('DC_TRACE_DECONV_SEARCH_SMIN 0', 'DC_TRACE_DECONV_SEARCH_LAM 1', 'DC_TRACE_DECONV_SEARCH_MAX_ROUNDS 64',
                 'DC_TRACE_DECONV_SEARCH_MAX_GROUPS 8192'):
        assert text in header, text
    assert deconv.CONSTRAIN == {'s_min': sr.SMIN, 'lam': sr.LAM} and deconv.MAX_ROUNDS == 64 and deconv.MAX_SIGMA == 2.0 ** 500
    assert deconv.SEARCH_KINDS == ('param', 'rss', 'target', 'status')
    math_h = open(os.path.join(ROOT, 'deep_calcium_amd', 'csrc', 'deconv_search_math.h')).read()
    assert '#pragma clang fp contract(off)' in math_h


def test_the_fold_is_the_one_of_the_trace_dynamics():
    import _dyn_ref
    rs = np.random.RandomState(3)
    for n in (0, 1, 2, 255, 256, 257, 1000):
        x = rs.standard_normal(n).tolist()
        assert sr.fold(x) == _dyn_ref.fold(x)


# ---- the host entry point -----------------------------------------------------------------------------------------------------------
def _rows(T, seed):
    """Events on noise held to their own noise, and pure noise around zero held to twice its level."""
    rs = np.random.RandomState(seed)
    sp = rs.poisson(0.05, T) > 0
    a = np.convolve(sp, np.exp(-np.arange(T) / 8.0))[:T] + 0.25 * rs.standard_normal(T)
    b = 0.3 * rs.standard_normal(T)
    return np.stack([a, b]), np.array([0.25, 0.6])


@pytest.mark.parametrize('T', (1, 2, 3, 255, 256, 257, 600))
def test_host_entry_equals_the_oracle_bit_for_bit(dclib, T):
    y64, sigma = _rows(T, T)
    for which in (sr.SMIN, sr.LAM):
        for rounds in (1, 5, 24):
            for dtype, pad, g, other in ((np.float32, 0, G8, 0.0), (np.float64, 0, math.exp(-1.0 / 30), 0.0), (np.float32, 3, math.exp(-1.0 / 2), 0.1),
                                         (np.float64, 3, G8, 0.05)):
                y = y64.astype(dtype)
                want = sr.deconvolve(y, g, which, sigma, other, rounds)
                got = sr.host_entry(dclib, y, g, which, sigma, other, rounds, pad=pad)
                for name in sr.NAMES:
                    assert ref.same_bits(got[name], want[name]), (name, T, which, rounds, dtype.__name__, pad)
                assert (got['param'] >= 0).all() and not np.signbit(got['calcium']).any()


def test_the_statuses_constructed(dclib):
    T = 600
    sp, noisy = ref.reach_trace(1, 0.3, T)
    clean = np.convolve(sp, np.exp(-np.arange(T) / 8.0))[:T][None]
    # sigma = 0: the target is 0 and no residual is below it
    got = sr.host_entry(dclib, clean, G8, sr.SMIN, 0.0)
    assert got['status'].tolist() == [1] and got['param'].tolist() == [0.0]
    assert ref.same_bits(got['calcium'], ref.deconvolve(clean, G8)[0]) and got['rss'][0] == sr.rss(clean[0].tolist(), ref.table(G8, T), sr.SMIN, 0.0, 0.0)
    # a tiny sigma: whatever the oracle says.  RSS(0) of the noiseless train is rounding only, below any such target, so the search
    # starts; the first value tried is sigma itself and amplitude-1 events only give way to a threshold near 1, which takes
    # log2(1 / sigma) doublings: 64 rounds bracket (status 0), the default 24 cannot from 1e-9 (status 2, still slack)
    for sigma in (1e-9, 1e-5):
        for which in (sr.SMIN, sr.LAM):
            for rounds, allowed in ((64, (0, 1)), (24, (0, 1, 2))):
                got, want = sr.host_entry(dclib, clean, G8, which, sigma, 0.0, rounds), sr.deconvolve(clean, G8, which, sigma, 0.0, rounds)
                assert got['status'].tolist() == want['status'].tolist() and got['status'][0] in allowed, (sigma, which, rounds)
                assert all(ref.same_bits(got[k], want[k]) for k in sr.NAMES)
    assert sr.host_entry(dclib, clean, G8, sr.SMIN, 1e-9, 0.0, 24)['status'].tolist() == [2]
    # all zero: RSS is 0 for every p, the search doubles to the end
    zero = np.zeros((1, T), np.float32)
    for rounds in (1, 2, 7, 24, 64):
        for which in (sr.SMIN, sr.LAM):
            got = sr.host_entry(dclib, zero, G8, which, 1.0, 0.0, rounds)
            assert got['status'].tolist() == [2] and got['param'].tolist() == [2.0 ** (rounds - 1)] and got['rss'].tolist() == [0.0]
            assert got['calcium'].tobytes() == np.zeros(T).tobytes() and sr.search(zero[0], ref.table(G8, T), which, 1.0, 0.0, rounds)['status'] == 2
    # a reach trace: bracketed
    from deep_calcium_amd.deconv import trace_noise
    got = sr.host_entry(dclib, noisy[None], G8, sr.SMIN, trace_noise(noisy[None]))
    assert got['status'].tolist() == [0] and got['param'][0] > 0


def test_invariants_on_the_reach_traces(dclib):
    """40 traces at sigma 0.3, s_min searched: RSS(p*) recomputed by the oracle is within the target; where the search bracketed,
    the oracle's RSS(hi) is beyond it and the bracket has the promised width; the outputs are those of the deconvolution at p*."""
    from deep_calcium_amd.deconv import trace_noise
    y = np.stack([ref.reach_trace(seed, 0.3)[1] for seed in range(40)])
    sigma = trace_noise(y)
    got = sr.host_entry(dclib, y, G8, sr.SMIN, sigma)
    G = ref.table(G8, y.shape[1])
    for r in range(40):
        row = [float(v) for v in y[r]]
        s = sr.search(row, G, sr.SMIN, sigma[r])
        assert (s['param'], s['rss'], s['status']) == (got['param'][r], got['rss'][r], got['status'][r])
        assert sr.rss(row, G, sr.SMIN, s['param'], 0.0) == s['rss'] <= s['target']
        assert s['status'] == 0                                                          # every reach trace brackets
        assert sr.rss(row, G, sr.SMIN, s['hi'], 0.0) > s['target']
        e = sum(1 for (p, _, _, _), (_, _, _, hi) in zip(s['trail'][1:], s['trail']) if p == hi)     # rounds that tried hi itself
        assert abs((s['hi'] - s['param']) - sigma[r] * 2.0 ** (max(e - 2, 0) - (24 - e))) <= 24 * 2.0 ** -52 * s['hi']
    want = ref.deconvolve(y, G8, smin=got['param'])
    for name, b in zip(('calcium', 'spikes', 'pools'), want):
        assert ref.same_bits(got[name], b), name


# ---- validation ---------------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    from deep_calcium_amd import _lib
    from deep_calcium_amd.deconv import TraceDeconvolver, deconvolve_traces_device

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'lib', boom)
    y = np.arange(12, dtype=np.float32).reshape(2, 6)
    for kw, what in ((dict(constrain='smin'), "constrain must be None, 's_min' or 'lam'"),
                     (dict(constrain=0), "constrain must be None, 's_min' or 'lam'"),
                     (dict(constrain='s_min', s_min=0.1), 's_min is searched'),
                     (dict(constrain='s_min', s_min=[0.0, 0.2]), 's_min is searched'),
                     (dict(constrain='lam', lam=0.5), 'lam is searched'),
                     (dict(constrain='s_min', rounds=0), r'rounds must be an integer in \[1, 64\]'),
                     (dict(constrain='s_min', rounds=65), r'rounds must be an integer in \[1, 64\]'),
                     (dict(constrain='lam', rounds=2.5), r'rounds must be an integer in \[1, 64\]'),
                     (dict(constrain='lam', rounds=True), r'rounds must be an integer in \[1, 64\]'),
                     (dict(constrain='s_min', sigma=-0.1), 'sigma must be finite and >= 0: trace 0'),
                     (dict(constrain='s_min', sigma=[0.1, float('nan')]), 'sigma must be finite and >= 0: trace 1'),
                     (dict(constrain='s_min', sigma=float('inf')), 'sigma must be finite'),
                     (dict(constrain='s_min', sigma=2.0 ** 500), r'sigma must be below 2\*\*500: trace 0'),
                     (dict(constrain='lam', sigma=[1.0, 2.0 ** 600]), r'sigma must be below 2\*\*500: trace 1'),
                     (dict(constrain='s_min', sigma=[0.1, 0.2, 0.3]), 'sigma must be a scalar or one value per trace'),
                     (dict(constrain='s_min', sigma=np.zeros((2, 1))), 'sigma must be a scalar or one value per trace'),
                     (dict(constrain='s_min', sigma='x'), 'sigma must be a number'),
                     (dict(sigma=0.1), 'needs constrain=')):
        with pytest.raises(ValueError, match=what):
            TraceDeconvolver(y, 0.9, **kw)
    nowhere = '/nonexistent/dataset.npz'
    ok = [np.array([[1, 2], [3, 4]])]
    for k in ('auto', 'Noise', ''):
        with pytest.raises(ValueError, match="k must be a number >= 0 or 'noise'"):
            deconvolve_traces_device(nowhere, ok, window=3, tau=1.0, fps=30, k=k)
    with pytest.raises(ValueError, match='tau and fps'):                           # k='noise' passes that check; the next one refuses
        deconvolve_traces_device(nowhere, ok, window=3, tau=0.0, fps=30, k='noise')


def test_new_kinds_on_an_unconstrained_object_raise_as_before():
    from deep_calcium_amd.deconv import KINDS, _check_kind
    for kind in ('param', 'rss', 'target', 'status', 'nothing'):
        with pytest.raises(ValueError, match='deconvolution kind %r is not one of calcium, spikes, pools' % kind):
            _check_kind(kind)
        with pytest.raises(ValueError, match='is not one of calcium, spikes, pools'):
            _check_kind(kind, constrained=False)
    for kind in KINDS + ('param', 'rss', 'target', 'status'):
        _check_kind(kind, constrained=True)
    with pytest.raises(ValueError, match='is not one of'):
        _check_kind('nothing', constrained=True)


def test_c_abi_argument_validation_returns_codes(dclib):
    """Refused before any launch (there is no GPU here); the device entry point never follows its pointers."""
    from deep_calcium_amd._lib import DcunetError
    p = 4096                                  # any aligned non-null value
    dev = dclib.dc_trace_deconv_ar1_constrained
    #     y  f64 ld R  T  g    gs    G  ldG which sigma other rounds ws state c  s  pools param rss status stream
    ok = [p, 0, 8, 2, 8, 0.9, None, p, 0, 0, p, p, 24, p, p, p, p, p, p, p, p, None]
    for i in (0, 7, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20):
        with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
            dev(*[None if j == i else a for j, a in enumerate(ok)])
    for i in (7, 10, 11, 13, 14, 15, 16, 18, 19):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            dev(*[a + 4 if j == i else a for j, a in enumerate(ok)])
    for i in (0, 17, 20):
        with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
            dev(*[a + 2 if j == i else a for j, a in enumerate(ok)])
    for which in (-1, 2):
        with pytest.raises(DcunetError, match=r'\(-1\).*which = %d' % which):
            dev(*[which if j == 9 else a for j, a in enumerate(ok)])
    for rounds in (0, 65, -3):
        with pytest.raises(DcunetError, match=r'\(-1\).*rounds = %d is outside \[1, 64\]' % rounds):
            dev(*[rounds if j == 12 else a for j, a in enumerate(ok)])
    for g in (0.0, 1.0, float('nan')):
        with pytest.raises(DcunetError, match=r'\(-1\).*outside \(0, 1\)'):
            dev(*[g if j == 5 else a for j, a in enumerate(ok)])
    with pytest.raises(DcunetError, match=r'\(-1\).*ldG = 8 is below T \+ 1 = 9'):
        dev(*[p if j == 6 else 8 if j == 8 else a for j, a in enumerate(ok)])
    with pytest.raises(DcunetError, match=r'\(-1\).*ld = 7 is below T = 8'):
        dev(*[7 if j == 2 else a for j, a in enumerate(ok)])
    big = (1 << 24) + 1
    with pytest.raises(DcunetError, match=r'\(-3\).*T = %d is over the limit' % big):
        dev(*[big if j in (2, 4) else 1 if j == 3 else a for j, a in enumerate(ok)])
    assert dev(*[0 if j == 3 else a for j, a in enumerate(ok)]) == 0 and dev(*[0 if j == 4 else a for j, a in enumerate(ok)]) == 0
    assert dev(*[0 if j == 3 else p if j == 6 else 9 if j == 8 else 0.0 if j == 5 else a for j, a in enumerate(ok)]) == 0      # per trace: g is not used
    nbytes = dclib.dc_trace_deconv_search_state_bytes
    assert nbytes(1) == 40 and nbytes(4096) == 40 * 4096 and nbytes(0) == 0 and nbytes(-1) == 0
    # the host entry point checks what it reads
    y = np.zeros((2, 8), np.float32)
    for kw, what in ((dict(sigma=[0.1, -1.0]), r'trace 1: sigma'), (dict(sigma=[float('nan'), 0.1]), r'trace 0: sigma'),
                     (dict(sigma=[0.1, 2.0 ** 500]), r'trace 1: sigma'), (dict(other=[-0.5, 0.0]), r'trace 0: the fixed parameter'),
                     (dict(rounds=0), 'rounds = 0'), (dict(which=3), 'which = 3')):
        a = dict(sigma=0.1, other=0.0, rounds=24, which=0)
        a.update(kw)
        with pytest.raises(DcunetError, match=r'\(-1\).*' + what):
            sr.host_entry(dclib, y, 0.9, a['which'], a['sigma'], a['other'], a['rounds'])


def test_example_refuses_spike_constrain_with_spike_k():
    script = os.path.join(ROOT, 'examples', 'neurons', 'unet2ds_nf.py')
    base = [sys.executable, script, 'traces', 'nowhere.npz', '-m', 'nowhere.hdf5', '--dff', '101', '--deconvolve', 'auto']
    for extra, what in ((['--spike-constrain', 's_min', '--spike-k', '2'], 'not together with --spike-k'),
                        (['--spike-k=3', '--spike-constrain', 'lam'], 'not together with --spike-k')):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and what in r.stderr, (extra, r.stderr[-500:])
    r = subprocess.run(base[:-4] + ['--spike-constrain', 's_min'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and '--spike-constrain needs --deconvolve' in r.stderr, r.stderr[-500:]


# ---- reach ---------------------------------------------------------------------------------------------------------------------------
def test_reach_of_the_searched_threshold(dclib, capsys):
    """What the search buys: the generator and the matching of tests/test_deconv_api.py, 40 seeds of T = 1024, true g = exp(-1/8), a
    hit within +-2 frames; s_min = k sigma_hat for k = 2 and 3 against s_min searched to RSS <= sigma_hat^2 T in 24 rounds (the
    library's host entry point, equal to the oracle in every bit by the tests above), and lam searched the same way, whose
    s > 0 is printed and not asserted: the L1 solution is a denoised calcium, not an event detector.  Asserted: the searched s_min is
    no more than 0.08 F1 below the better fixed k at sigma 0.1, 0.2 and 0.3, and at least 0.10 above both at sigma 0.5, where
    every fixed k collapses.  A scratch run with a plain sum for the fold measured gaps of 0.003, 0.029, 0.056 and a margin of 0.18."""
    from deep_calcium_amd.deconv import trace_noise
    rows = {}
    for sigma in (0.1, 0.2, 0.3, 0.5):
        pairs = [ref.reach_trace(seed, sigma) for seed in range(40)]
        y = np.stack([p[1] for p in pairs])
        sig = trace_noise(y)
        spikes = {'k = 2': ref.host_entry(dclib, y, G8, 0.0, 2.0 * sig)[1], 'k = 3': ref.host_entry(dclib, y, G8, 0.0, 3.0 * sig)[1]}
        found = sr.host_entry(dclib, y, G8, sr.SMIN, sig)
        l1 = sr.host_entry(dclib, y, G8, sr.LAM, sig)
        spikes['s_min searched'], spikes['lam searched'] = found['spikes'], l1['spikes']
        cells = {}
        for name, s in spikes.items():
            tot = np.zeros(3, int)
            for r, (sp, _) in enumerate(pairs):
                true, ev = np.flatnonzero(sp), np.flatnonzero(s[r] > 0)
                tot += (ref.match(true, ev), len(true), len(ev))
            cells[name] = ref.prf(*tot)
        ratio = found['param'] / sig
        rows[sigma] = (cells, (ratio.min(), np.median(ratio), ratio.max()), np.bincount(found['status'], minlength=3))
    with capsys.disabled():
        print('\n  sigma  k = 2                  k = 3                  s_min searched         lam searched           s_min / sigma_hat found   status 0 / 1 / 2')
        for sigma, (cells, ratio, counts) in rows.items():
            print('  %.1f    %s   %.2f / %.2f / %.2f        %d / %d / %d' % (
                sigma, '  '.join('%.3f / %.3f / %.3f' % cells[n] for n in ('k = 2', 'k = 3', 's_min searched', 'lam searched')),
                ratio[0], ratio[1], ratio[2], counts[0], counts[1], counts[2]))
    f1 = lambda sigma, name: rows[sigma][0][name][2]                            # noqa: E731
    assert f1(0.5, 's_min searched') >= max(f1(0.5, 'k = 2'), f1(0.5, 'k = 3')) + 0.10
    for sigma in (0.1, 0.2, 0.3):
        assert f1(sigma, 's_min searched') >= max(f1(sigma, 'k = 2'), f1(sigma, 'k = 3')) - 0.08, sigma


# ---- the shared arithmetic ---------------------------------------------------------------------------------------------------------
def test_deconv_search_math_under_the_host_sanitizers(tmp_path):
    """csrc/deconv_search_math.h compiled into tests/native/deconv_search_check.cpp with the address and undefined-behaviour
    sanitizers and run as a program of its own: the step against a model residual, and the host search over ragged T with buffers
    exactly T long."""
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
    exe = str(tmp_path / 'deconv_search_check')
    src = os.path.join(ROOT, 'tests', 'native', 'deconv_search_check.cpp')
    r = subprocess.run([cxx] + flags + [src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'deconv_search_check: ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
