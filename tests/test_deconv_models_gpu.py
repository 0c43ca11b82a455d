"""Every instantiation of the deconvolution kernels once (csrc/deconv.hip: the forward kernel over input type x model source x
baseline, the fill over the model source, the sweep over input type x model source, with a baseline for AR(1) only): the entry
points of the three model sources -- AR(1) with one decay, AR(1) with a decay per trace, AR(2) -- on float32 and float64 rows,
without and with a baseline, against the plain-Python oracles in every bit.  The other test files reach only part of that grid
(tests/test_deconv_base_gpu.py pairs float32 with one decay and float64 with a decay per trace, for one).  R = 65, T = 67: two
workgroups of the forward kernel, the second with one live lane, and two frame tiles, the second of three frames.  The helpers
are those of the files that test each entry point at length; they pre-fill outputs and workspace with NaN or canaries."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _deconv_ar2_ref as a2            # noqa: E402
import _deconv_base_ref as br           # noqa: E402
import _deconv_ref as ref               # noqa: E402
import _deconv_search_ref as sr         # noqa: E402
import test_deconv_ar2_gpu as ar2       # noqa: E402
import test_deconv_base_gpu as based    # noqa: E402
import test_deconv_gpu as plain         # noqa: E402
import test_deconv_search_gpu as search # noqa: E402
import test_dynamics_gpu as dyn         # noqa: E402

R, T = 65, 67
ROOTS = a2.ROOTS[1]
SOURCES = ('one', 'each', 'ar2')
INPUTS = ((np.float32, 3), (np.float64, 0))                                 # (dtype, pad): ld = T + 3 with NaN padding, ld = T
THREE = ('calcium', 'spikes', 'pools')


@pytest.fixture(scope='module')
def L(dclib):
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return dclib


def _decay(source):
    """One decay for all traces, or one per trace, three distinct ones among the lanes of a wave."""
    return plain.GAMMAS[1] if source == 'one' else np.array([plain.GAMMAS[(r // 4) % 3] for r in range(R)])


def _same(got, want, what, names):
    if not isinstance(got, dict):
        got, want = dict(zip(THREE, got)), dict(zip(THREE, want))
    for name in names:
        a, b = got[name], want[name]
        assert not np.isnan(a).any() if a.dtype.kind == 'f' else (a >= 0).all(), (name, what)
        assert ref.same_bits(a, b), (name, what, np.argwhere(a != b)[:5].tolist())


@pytest.mark.parametrize('dtype, pad', INPUTS, ids=('float32', 'float64'))
@pytest.mark.parametrize('source', SOURCES)
def test_the_plain_entry_points_over_the_grid(L, source, dtype, pad):
    """dc_trace_deconv_ar1, _ar1_each, _ar1_base (one decay, one per trace) and _ar2 (without and with a baseline): the forward
    kernel <In, source, Base> and the fill <source>."""
    y = plain._traces(R, T, 11).astype(dtype)
    lam, smin = plain._penalties(R, 11)
    base = 0.3 * np.random.RandomState(13).standard_normal(R)
    what = (source, dtype.__name__)
    if source == 'ar2':
        d, r = ROOTS
        _same(ar2._device_run(L, y, d, r, lam, smin, None, pad=pad), a2.deconvolve(y, d, r, lam, smin, None), what + ('no baseline',), THREE)
        _same(ar2._device_run(L, y, d, r, lam, smin, base, pad=pad), a2.deconvolve(y, d, r, lam, smin, base), what + ('baseline',), THREE)
        return
    g = _decay(source)
    if source == 'one':
        got = plain._device_run(L, y, g, lam, smin, pad=pad)
    else:
        got, _ = dyn._device_deconv_each(L, y, g, lam, smin, pad=pad)
    _same(dict(zip(THREE, got)), br.deconvolve(y, g, lam, smin, 0.0, 0), what + ('no baseline',), THREE)
    _same(based._Device(L, y, g, pad).given(lam, smin, base), br.deconvolve(y, g, lam, smin, base, 0), what + ('baseline',), br.FIT_NAMES)


@pytest.mark.parametrize('dtype, pad', INPUTS, ids=('float32', 'float64'))
@pytest.mark.parametrize('source', SOURCES)
def test_the_searches_over_the_grid(L, source, dtype, pad):
    """dc_trace_deconv_ar1_constrained and _ar2_constrained in 3 rounds, `which` alternating over the grid: the plain sweep
    <In, source>.  For AR(1) also _ar1_constrained_base in 3 rounds and _ar1_fit_base in 2: the sweep with a baseline."""
    which = (sr.SMIN, sr.LAM)[(SOURCES.index(source) + pad) % 2]
    other = 0.05
    what = (source, dtype.__name__, which)
    if source == 'ar2':
        d, r = ROOTS
        y64, sigma = ar2._mixed(R, T, 17, d, r)
        y = y64.astype(dtype)
        a2.same(ar2._device_search(L, y, d, r, which, sigma, other, 3, pad=pad), a2.constrained(y, d, r, which, sigma, other, 3), what, search.SEVEN)
        return
    g = _decay(source)
    y64, sigma = search._mixed(R, T, 17)
    y = y64.astype(dtype)
    _same(search._device_run(L, y, g, which, sigma, other, 3, pad=pad), sr.deconvolve(y, g, which, sigma, other, 3), what, search.SEVEN)
    y64, sigma = based._mixed(R, T, 19)
    y = y64.astype(dtype)
    b0 = np.where(np.arange(R) % 3 == 0, 0.0, 0.1 * np.sin(np.arange(R)))
    dev = based._Device(L, y, g, pad)
    _same(dev.search(which, sigma, other, b0, 3), br.deconvolve_search(y, g, which, sigma, other, b0, 3), what + ('baseline',), based.EIGHT)
    lam, smin = (other, 0.3 * sigma) if which == sr.SMIN else (0.2 * sigma, other)
    _same(dev.fit(lam, smin, b0, 2), br.deconvolve(y, g, lam, smin, b0, 2), what + ('fit',), br.FIT_NAMES)
