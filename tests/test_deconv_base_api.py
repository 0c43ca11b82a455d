"""A baseline in the deconvolution, without a GPU: the public names and the ABI, the library's host entry points against the
plain-Python oracle (tests/_deconv_base_ref.py) bit for bit, baseline = 0 and a given baseline against the entry points that have
none, the promise RSS(p*, b*) <= target, a constant trace and T = 1, argument validation in front of the library, the reach table
on the dF/F the chain produces, and csrc/deconv_base_math.h as a stand-alone program under the host sanitizers."""
import math
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import _deconv_base_ref as br
import _deconv_ref as ref
import _deconv_search_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G8 = math.exp(-1.0 / 8)
GAMMAS = (math.exp(-1.0 / 2), G8, math.exp(-1.0 / 30))


def test_public_names_and_abi():
    from deep_calcium_amd import _build, _gen_tape, _lib, deconv
    assert _lib.header_abi_version() >= 129
    protos = _lib.parse_header()
    names = ('dc_trace_deconv_base_state_bytes', 'dc_trace_deconv_ar1_base', 'dc_trace_deconv_ar1_fit_base', 'dc_trace_deconv_ar1_constrained_base',
             'dc_trace_deconv_base_step', 'dc_trace_deconv_ar1_fit_base_host', 'dc_trace_deconv_ar1_constrained_base_host')
    assert [len(protos[n][1]) for n in names] == [1, 17, 18, 23, 17, 14, 18]
    assert set(names[1:]) <= set(n for n, _ in _gen_tape.prototypes())
    header = open(_lib.HEADER).read()
    for text in ('DC_TRACE_DECONV_BASE_MAX_ROUNDS 64', 'DC_TRACE_DECONV_BASE_FIT 0', 'DC_TRACE_DECONV_BASE_PASS_A 1', 'DC_TRACE_DECONV_BASE_PASS_B 2',
                 'DC_TRACE_DECONV_BASE_PASS_LAST 3'):
        assert text in header, text
    assert deconv.MAX_BASELINE_ROUNDS == 64 and (br.FIT, br.PASS_A, br.PASS_B, br.PASS_LAST) == (0, 1, 2, 3)
    math_h = open(os.path.join(ROOT, 'deep_calcium_amd', 'csrc', 'deconv_base_math.h')).read()
    assert '#pragma clang fp contract(off)' in math_h and '-ffp-contract=off' in _build.FILE_FLAGS['deconv.hip']


# ---- the host entry points -----------------------------------------------------------------------------------------------------------
def _rows(T, seed):
    """Events on noise above an offset, the same at half the size on another offset, pure noise around an offset, a constant row."""
    rs = np.random.RandomState(seed)
    sp = rs.poisson(0.05, T) > 0
    a = np.convolve(sp, np.exp(-np.arange(T) / 8.0))[:T] + 0.25 * rs.standard_normal(T) + 0.3
    b = 0.5 * a - 0.4
    c = 0.3 * rs.standard_normal(T) + 0.2
    return np.stack([a, b, c, np.full(T, 0.75)]), np.array([0.25, 0.125, 0.6, 1.0])


@pytest.mark.parametrize('T', (1, 2, 3, 255, 256, 257, 600))
def test_host_entries_equal_the_oracle_bit_for_bit(dclib, T):
    """Both `which`, a scalar decay and one per trace, float32 and float64, rows and table rows padded with NaN; the fit at 0 (the
    given baseline), 1 and 5 rounds from a start per trace, the joint search at 1 and 6 rounds."""
    y64, sigma = _rows(T, T)
    g_each = np.array([GAMMAS[(r + T) % 3] for r in range(4)])
    b0 = np.array([0.0, -0.1, 0.2, 0.5])
    for dtype, pad, g, other in ((np.float32, 0, G8, 0.0), (np.float64, 3, g_each, 0.05), (np.float32, 3, g_each, 0.0), (np.float64, 0, GAMMAS[2], 0.1)):
        y = y64.astype(dtype)
        what = (T, dtype.__name__, pad, np.ndim(g))
        for rounds in (0, 1, 5):
            want = br.deconvolve(y, g, other, 0.3, b0, rounds)
            got = br.host_fit(dclib, y, g, other, 0.3, b0, rounds, pad=pad)
            for name in br.FIT_NAMES:
                assert ref.same_bits(got[name], want[name]), (name, rounds) + what
        for which in (br.SMIN, br.LAM):
            for rounds, start in ((1, 0.0), (6, b0)):
                want = br.deconvolve_search(y, g, which, sigma, other, start, rounds)
                got = br.host_search(dclib, y, g, which, sigma, other, start, rounds, pad=pad)
                for name in br.SEARCH_NAMES:
                    assert ref.same_bits(got[name], want[name]), (name, which, rounds) + what
                assert (got['param'] >= 0).all() and not np.signbit(got['calcium']).any()


def test_baseline_zero_gives_the_bits_of_the_entry_points_without_one(dclib):
    """z - 0.0 is z for every double: the given baseline 0 is dc_trace_deconv_ar1_host, and a joint search whose baseline cannot
    move -- an all-zero row: S = 0 in every round -- is dc_trace_deconv_ar1_constrained_host."""
    y = np.stack([ref.reach_trace(seed, 0.3, 600)[1] for seed in range(6)])
    y[5, ::7] = -0.0
    for dtype in (np.float32, np.float64):
        old = ref.host_entry(dclib, y.astype(dtype), G8, 0.05, 0.4)
        new = br.host_fit(dclib, y.astype(dtype), G8, 0.05, 0.4, 0.0, 0)
        for name, b in zip(('calcium', 'spikes', 'pools'), old):
            assert ref.same_bits(new[name], b), (name, dtype.__name__)
        assert new['baseline'].tobytes() == np.zeros(6).tobytes()
    zero = np.zeros((1, 300), np.float32)
    for which in (br.SMIN, br.LAM):
        old, new = sr.host_entry(dclib, zero, G8, which, 1.0, 0.0, 9), br.host_search(dclib, zero, G8, which, 1.0, 0.0, 0.0, 9)
        for name in sr.NAMES:
            assert ref.same_bits(new[name], old[name]), (name, which)
        assert new['baseline'].tolist() == [0.0] and new['status'].tolist() == [2]


def test_a_given_baseline_is_the_entry_point_without_one_on_y_minus_b(dclib):
    """(double)y[t] - b is formed once, in float64, and the rest of the forward pass is the old one: the bits of
    dc_trace_deconv_ar1_host run on y - b precomputed in float64, for float32 and float64 input."""
    y = np.stack([ref.reach_trace(seed, 0.2, 500)[1] for seed in range(5)])
    b = np.array([0.0, 0.21, -0.3, 1e-3, 0.137])
    for dtype in (np.float32, np.float64):
        new = br.host_fit(dclib, y.astype(dtype), G8, 0.02, 0.35, b, 0, pad=2)
        old = ref.host_entry(dclib, y.astype(dtype).astype(np.float64) - b[:, None], G8, 0.02, 0.35)
        for name, want in zip(('calcium', 'spikes', 'pools'), old):
            assert ref.same_bits(new[name], want), (name, dtype.__name__)
        assert ref.same_bits(new['baseline'], b)


def test_the_promise_on_the_dff_traces(dclib):
    """16 dF/F traces at sigma 0.3, s_min and the baseline searched jointly: RSS(p*, b*) re-evaluated by the oracle at exactly that
    pair is the one reported and within the target; the bracket has the plain search's width; the outputs are those of the given
    baseline b* at the threshold p*."""
    from deep_calcium_amd.deconv import trace_noise
    y = np.stack([br.reach_dff(seed, 0.3)[1] for seed in range(16)])
    sigma = trace_noise(y)
    got = br.host_search(dclib, y, G8, br.SMIN, sigma)
    G = ref.table(G8, y.shape[1])
    for r in range(16):
        row = [float(v) for v in y[r]]
        s = br.search(row, G, br.SMIN, sigma[r])
        assert (s['param'], s['base'], s['rss'], s['status']) == (got['param'][r], got['baseline'][r], got['rss'][r], got['status'][r])
        assert br.sums(row, G, br.forward(row, G, 0.0, s['param'], s['base']), s['base'])[0] == s['rss'] <= s['target']
        assert s['status'] == 0
        e = sum(1 for now, before in zip(s['trail'][1:], s['trail']) if now[0] == before[4])        # rounds that tried hi itself
        assert abs((s['hi'] - s['param']) - sigma[r] * 2.0 ** (max(e - 2, 0) - (24 - e))) <= 24 * 2.0 ** -52 * s['hi']
    given = br.host_fit(dclib, y, G8, 0.0, got['param'], got['baseline'], 0)
    for name in ('calcium', 'spikes', 'pools'):
        assert ref.same_bits(got[name], given[name]), name


def test_a_constant_trace_and_one_frame(dclib):
    """A constant row: the fit finds the constant in one step while the trace has no pool above zero (A = 0: b' = b + mean
    residual); T = 1: whatever the oracle says, in every bit, and no frame beyond the first is touched."""
    flat = np.full((1, 300), 0.75)
    for T in (1, 2, 300):
        y = flat[:, :T]
        got = br.host_fit(dclib, y, G8, 0.0, 0.0, 1.0, 1)                  # from above: y - b < 0, every pool is below zero
        assert got['baseline'].tolist() == [0.75] and not got['calcium'].any() and not got['spikes'].any()
        for which in (br.SMIN, br.LAM):
            for b0 in (0.0, 1.0):
                want, have = br.deconvolve_search(y, G8, which, 1.0, 0.0, b0, 5), br.host_search(dclib, y, G8, which, 1.0, 0.0, b0, 5)
                assert all(ref.same_bits(have[k], want[k]) for k in br.SEARCH_NAMES), (T, which, b0)
                assert have['status'][0] == 1 or have['rss'][0] <= 1.0 * T
    one = np.array([[0.3]], np.float32)
    want, have = br.deconvolve(one, G8, 0.1, 0.0, 0.0, 3), br.host_fit(dclib, one, G8, 0.1, 0.0, 0.0, 3, pad=4)
    assert all(ref.same_bits(have[k], want[k]) for k in br.FIT_NAMES)


# ---- validation ---------------------------------------------------------------------------------------------------------------------
def test_arguments_are_checked_before_the_library_is_touched(monkeypatch):
    from deep_calcium_amd import _lib
    from deep_calcium_amd.deconv import TraceDeconvolver, deconvolve_traces_device

    def boom(*a, **k):
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'lib', boom)
    y = np.arange(12, dtype=np.float32).reshape(2, 6)
    for kw, what in ((dict(baseline='Fit'), "baseline must be a number, one value per trace or 'fit'"),
                     (dict(baseline=''), "baseline must be a number, one value per trace or 'fit'"),
                     (dict(baseline=[1.0, 'x']), "baseline must be a number, one value per trace or 'fit'"),
                     (dict(baseline=float('nan')), 'baseline must be finite: trace 0'),
                     (dict(baseline=[0.0, float('inf')]), 'baseline must be finite: trace 1'),
                     (dict(baseline=[0.1, 0.2, 0.3]), 'baseline must be a scalar or one value per trace'),
                     (dict(baseline=np.zeros((2, 1))), 'baseline must be a scalar or one value per trace'),
                     (dict(baseline='fit', baseline_rounds=0), r'baseline_rounds must be an integer in \[1, 64\]'),
                     (dict(baseline='fit', baseline_rounds=65), r'baseline_rounds must be an integer in \[1, 64\]'),
                     (dict(baseline='fit', baseline_rounds=2.0), r'baseline_rounds must be an integer in \[1, 64\]'),
                     (dict(baseline='fit', baseline_rounds=True), r'baseline_rounds must be an integer in \[1, 64\]'),
                     (dict(baseline=0.1, constrain='s_min'), 'a given baseline cannot go with constrain='),
                     (dict(baseline=[0.0, 0.0], constrain='lam'), 'a given baseline cannot go with constrain='),
                     (dict(baseline='fit', constrain='s_min', s_min=0.1), 's_min is searched')):
        with pytest.raises(ValueError, match=what):
            TraceDeconvolver(y, 0.9, **kw)
    nowhere = '/nonexistent/dataset.npz'
    ok = [np.array([[1, 2], [3, 4]])]
    for b, what in (('auto', "baseline must be a number"), ([0.0, 0.1], "baseline must be a scalar or 'fit' here"),
                    (float('inf'), 'baseline must be finite')):
        with pytest.raises(ValueError, match=what):
            deconvolve_traces_device(nowhere, ok, window=3, tau=1.0, fps=30, baseline=b)
    with pytest.raises(ValueError, match='a given baseline cannot go with constrain='):
        deconvolve_traces_device(nowhere, ok, window=3, tau=1.0, fps=30, k='noise', baseline=0.2)


def test_c_abi_argument_validation_returns_codes(dclib):
    """Refused before any launch (there is no GPU here); the device entry points never follow their pointers."""
    from deep_calcium_amd._lib import DcunetError
    p = 4096                                  # any aligned non-null value
    #      y  f64 ld R  T  g    gs    G  ldG lam smin base ws c  s  pools stream
    given = [p, 0, 8, 2, 8, 0.9, None, p, 0, p, p, p, p, p, p, p, None]
    #      y  f64 ld R  T  g    gs    G  ldG lam smin rounds ws c  s  pools base stream
    fit = [p, 0, 8, 2, 8, 0.9, None, p, 0, p, p, 8, p, p, p, p, p, None]
    #      y  f64 ld R  T  g    gs    G  ldG which sigma other rounds ws state c  s  pools param base rss status stream
    joint = [p, 0, 8, 2, 8, 0.9, None, p, 0, 0, p, p, 24, p, p, p, p, p, p, p, p, p, None]
    #      y  f64 ld R  T  G  ldG ws pools mode state param base rss status sums stream
    step = [p, 0, 8, 2, 8, p, 0, p, p, 2, p, p, p, p, p, None, None]
    for fn, ok, pointers, four in ((dclib.dc_trace_deconv_ar1_base, given, (0, 7, 9, 10, 11, 12, 13, 14, 15), (0, 15)),
                                   (dclib.dc_trace_deconv_ar1_fit_base, fit, (0, 7, 9, 10, 12, 13, 14, 15, 16), (0, 15)),
                                   (dclib.dc_trace_deconv_ar1_constrained_base, joint, (0, 7, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20, 21), (0, 17, 21)),
                                   (dclib.dc_trace_deconv_base_step, step, (0, 5, 7, 8, 10, 11, 12, 13, 14), (0, 8, 14))):
        for i in pointers:
            with pytest.raises(DcunetError, match=r'\(-1\).*null pointer'):
                fn(*[None if j == i else a for j, a in enumerate(ok)])
            with pytest.raises(DcunetError, match=r'\(-1\).*misaligned'):
                fn(*[a + (2 if i in four else 4) if j == i else a for j, a in enumerate(ok)])
        with pytest.raises(DcunetError, match=r'\(-1\).*ld = 7 is below T = 8'):
            fn(*[7 if j == 2 else a for j, a in enumerate(ok)])
        big = (1 << 24) + 1
        with pytest.raises(DcunetError, match=r'\(-3\).*T = %d is over the limit' % big):
            fn(*[big if j in (2, 4) else 1 if j == 3 else a for j, a in enumerate(ok)])
        assert fn(*[0 if j == 3 else a for j, a in enumerate(ok)]) == 0 and fn(*[0 if j == 4 else a for j, a in enumerate(ok)]) == 0
    for fn, ok in ((dclib.dc_trace_deconv_ar1_base, given), (dclib.dc_trace_deconv_ar1_fit_base, fit), (dclib.dc_trace_deconv_ar1_constrained_base, joint)):
        for g in (0.0, 1.0, float('nan')):
            with pytest.raises(DcunetError, match=r'\(-1\).*outside \(0, 1\)'):
                fn(*[g if j == 5 else a for j, a in enumerate(ok)])
        with pytest.raises(DcunetError, match=r'\(-1\).*ldG = 8 is below T \+ 1 = 9'):
            fn(*[p if j == 6 else 8 if j == 8 else a for j, a in enumerate(ok)])
        assert fn(*[0 if j == 3 else p if j == 6 else 9 if j == 8 else 0.0 if j == 5 else a for j, a in enumerate(ok)]) == 0      # per trace: g is not used
    for rounds in (0, 65, -3):
        with pytest.raises(DcunetError, match=r'\(-1\).*rounds = %d is outside \[1, 64\]' % rounds):
            dclib.dc_trace_deconv_ar1_fit_base(*[rounds if j == 11 else a for j, a in enumerate(fit)])
        with pytest.raises(DcunetError, match=r'\(-1\).*rounds = %d is outside \[1, 64\]' % rounds):
            dclib.dc_trace_deconv_ar1_constrained_base(*[rounds if j == 12 else a for j, a in enumerate(joint)])
    for which in (-1, 2):
        with pytest.raises(DcunetError, match=r'\(-1\).*which = %d' % which):
            dclib.dc_trace_deconv_ar1_constrained_base(*[which if j == 9 else a for j, a in enumerate(joint)])
    for mode in (-1, 4):
        with pytest.raises(DcunetError, match=r'\(-1\).*mode = %d is outside \[0, 3\]' % mode):
            dclib.dc_trace_deconv_base_step(*[mode if j == 9 else a for j, a in enumerate(step)])
    with pytest.raises(DcunetError, match=r'\(-1\).*ldG = 8 is neither 0 nor at least T \+ 1 = 9'):
        dclib.dc_trace_deconv_base_step(*[8 if j == 6 else a for j, a in enumerate(step)])
    assert dclib.dc_trace_deconv_base_step(*[0 if j == 3 else None if j in (10, 11, 13, 14) else 0 if j == 9 else a for j, a in enumerate(step)]) == 0
    nbytes = dclib.dc_trace_deconv_base_state_bytes
    assert nbytes(1) == 56 and nbytes(4096) == 56 * 4096 and nbytes(0) == 0 and nbytes(-1) == 0
    # the host entry points check what they read
    y = np.zeros((2, 8), np.float32)
    for kw, what in ((dict(sigma=[0.1, -1.0]), r'trace 1: sigma'), (dict(sigma=[0.1, 2.0 ** 500]), r'trace 1: sigma'),
                     (dict(other=[-0.5, 0.0]), r'trace 0: the fixed parameter'), (dict(base=[0.0, float('nan')]), r'trace 1: the baseline'),
                     (dict(base=float('inf')), r'trace 0: the baseline'), (dict(rounds=0), 'rounds = 0'), (dict(which=3), 'which = 3')):
        a = dict(sigma=0.1, other=0.0, base=0.0, rounds=24, which=0)
        a.update(kw)
        with pytest.raises(DcunetError, match=r'\(-1\).*' + what):
            br.host_search(dclib, y, 0.9, a['which'], a['sigma'], a['other'], a['base'], a['rounds'])
    for kw, what in ((dict(lam=-0.1), r'trace 0: lam'), (dict(base=[0.0, float('-inf')]), r'trace 1: the baseline'), (dict(rounds=65), 'rounds = 65'),
                     (dict(rounds=-1), 'rounds = -1')):
        a = dict(lam=0.0, base=0.0, rounds=3)
        a.update(kw)
        with pytest.raises(DcunetError, match=r'\(-1\).*' + what):
            br.host_fit(dclib, y, 0.9, a['lam'], 0.0, a['base'], a['rounds'])


def test_example_takes_spike_baseline():
    script = os.path.join(ROOT, 'examples', 'neurons', 'unet2ds_nf.py')
    base = [sys.executable, script, 'traces', 'nowhere.npz', '-m', 'nowhere.hdf5', '--dff', '101']
    for extra, what in ((['--spike-baseline', 'fit'], '--spike-baseline needs --deconvolve'),
                        (['--deconvolve', 'auto', '--spike-baseline', 'Fit'], 'expected fit or a constant VALUE'),
                        (['--deconvolve', 'auto', '--spike-constrain', 's_min', '--spike-baseline', '0.1'], 'cannot go with --spike-constrain')):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 2 and what in r.stderr, (extra, r.stderr[-500:])


# ---- reach ---------------------------------------------------------------------------------------------------------------------------
def _totals(traces, spikes):
    tot = np.zeros(3, int)
    for r, (sp, _, _) in enumerate(traces):
        true, ev = np.flatnonzero(sp), np.flatnonzero(spikes[r] > 0)
        tot += (ref.match(true, ev), len(true), len(ev))
    return ref.prf(*tot)


def test_reach_on_the_dff_the_chain_produces(dclib, capsys):
    """The reach generator as the dF/F of this project: F = round(1000 (1 + y)), a running 8th percentile over 901 frames by the
    integer rank rule, (F - F0) / F0; 40 seeds of T = 1024, true g = exp(-1/8), a hit within +-2 frames, sigma_hat = trace_noise.
    s_min searched without a baseline against s_min and the baseline searched jointly (the library's host entry points, equal to
    the oracles in every bit by the tests above), and the fit at fixed k = 2 and 3 (baseline_rounds = 4) beside the same k without
    one.  Asserted at sigma 0.2 and 0.3: the joint F1 is at least the plain search's plus 0.15 (half of the gap of about 0.3 that
    8 seeds showed), and the median of b* / sigma_hat is within 0.25 of the median true offset -- the mean of dF/F over the frames
    whose true calcium is below 0.02 -- over sigma_hat.  Everything else is printed: sigma 0.5, and what the fixed-k fit does
    (it lifts a threshold that is too low and harms one that is too high, whose missed events go into the baseline)."""
    from deep_calcium_amd.deconv import trace_noise
    rows = {}
    for sigma in (0.2, 0.3, 0.5):
        traces = [br.reach_dff(seed, sigma) for seed in range(40)]
        y = np.stack([t[1] for t in traces])
        sig = trace_noise(y)
        plain = sr.host_entry(dclib, y, G8, sr.SMIN, sig)
        joint = br.host_search(dclib, y, G8, br.SMIN, sig)
        cells = {'searched': _totals(traces, plain['spikes']), 'joint': _totals(traces, joint['spikes'])}
        ratios = {'joint': joint['baseline'] / sig}
        for k in (2.0, 3.0):
            cells['k = %g' % k] = _totals(traces, ref.host_entry(dclib, y, G8, 0.0, k * sig)[1])
            fitted = br.host_fit(dclib, y, G8, 0.0, k * sig, 0.0, 4)
            cells['k = %g, fit' % k], ratios['k = %g, fit' % k] = _totals(traces, fitted['spikes']), fitted['baseline'] / sig
        offset = np.array([y[r][t[2] < 0.02].mean() for r, t in enumerate(traces)]) / sig
        rows[sigma] = (cells, ratios, offset, np.bincount(joint['status'], minlength=3))
    order = ('searched', 'joint', 'k = 2', 'k = 2, fit', 'k = 3', 'k = 3, fit')
    with capsys.disabled():
        print('\n  recall / precision / F1 on dF/F, 40 seeds')
        print('  sigma  ' + '  '.join('%-21s' % n for n in order))
        for sigma, (cells, ratios, offset, counts) in rows.items():
            print('  %.1f    %s' % (sigma, '  '.join('%.3f / %.3f / %.3f' % cells[n] for n in order)))
        print('  sigma  median b / sigma_hat: joint, k = 2 fit, k = 3 fit; median true offset / sigma_hat; joint status 0 / 1 / 2')
        for sigma, (cells, ratios, offset, counts) in rows.items():
            print('  %.1f    %.3f  %.3f  %.3f    %.3f    %d / %d / %d' % (sigma, np.median(ratios['joint']), np.median(ratios['k = 2, fit']),
                                                                        np.median(ratios['k = 3, fit']), np.median(offset), counts[0], counts[1], counts[2]))
    for sigma in (0.2, 0.3):
        cells, ratios, offset, _ = rows[sigma]
        assert cells['joint'][2] >= cells['searched'][2] + 0.15, (sigma, cells['joint'], cells['searched'])
        assert abs(np.median(ratios['joint']) - np.median(offset)) <= 0.25, (sigma, np.median(ratios['joint']), np.median(offset))


# ---- the shared arithmetic ---------------------------------------------------------------------------------------------------------
def test_deconv_base_math_under_the_host_sanitizers(tmp_path):
    """csrc/deconv_base_math.h compiled into tests/native/deconv_base_check.cpp with the address and undefined-behaviour sanitizers
    and run as a program of its own: the gain term and the step, the joint step against a model residual, and the host fit and
    search over ragged T with buffers exactly T long."""
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
    exe = str(tmp_path / 'deconv_base_check')
    src = os.path.join(ROOT, 'tests', 'native', 'deconv_base_check.cpp')
    r = subprocess.run([cxx] + flags + [src, '-o', exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'deconv_base_check: ok' in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
