"""The six grid-stride launches of the UNet1D kernels past their grid cap (DESIGN.md 4f-caps-1d has the table): spikes_blocks() clamps
the grid of dc_conv1d_k5_c1_fwd, dc_maxpool1d_2_fwd / _bwd and dc_upsample1d_2x_fwd / _drop_fwd / _drop_bwd at 8192 workgroups of 256
threads, and a thread strides over the rest.  The other modules stop at a few hundred items; default inference reaches a second trip
with every recording longer than 8192 samples.  Here every entry point runs a launch one item past the cap and one a little into its
third trip (tests/_caps1d.py has the shapes, tests/test_caps1d.py checks on the CPU that each lands in the regime claimed for it), and
UNet1DEngine runs one forward whose capped launches take two and three trips and whose uncapped ones tens of thousands of workgroups.

References are numpy or float64 written here or in tests/_unet1d_ref.py / _unet1d_train_ref.py, never the device itself.  Every
sample stride is C + 4 with the slice at channel offset 4, as the engine passes slices of its concat buffers; every output starts as
POISON with GUARD elements on both sides, and padding channels and guards must still be POISON afterwards.  What only moves values
(pooling, its routing plus one fp32 add, up-sampling, dropout at keep = 1/2, the kept positions of the counter RNG) is compared for
equality; the first layer on random data is held to the bound of test_spikes_gpu.py::test_conv1d_k5_c1_fwd and, because that bound
cannot see one misplaced sample among millions, to equality on integer-valued data.  A mismatch names the first wrong flat item and
its trip.  Every test prints the figure it asserts on."""
import time

import numpy as np
import pytest

from oracle import unet_numpy as on

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _caps1d as c1                  # noqa: E402
import _unet1d_ref as ref             # noqa: E402
import _unet1d_train_ref as tref      # noqa: E402

POISON = -12345.5                     # the value of test_spikes_train_gpu.py
GUARD = 8
PAD = c1.PAD
SEED = 0x5EED1DCAFEF00D
F32, F64 = np.float32, np.float64


@pytest.fixture(autouse=True)
def _release_device_memory():
    """The buffers here reach 150 MB each: hand them back, so that one test's cached blocks do not add to the next one's."""
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cases(entry):
    return pytest.mark.parametrize('case', c1.CASES[entry], ids=c1.case_ids(entry))


class _Out(object):
    """rows samples of ld floats, pre-filled with POISON, GUARD elements on both sides; the kernel is given the channel slice
    [ld - C, ld) of it.  host() synchronises, checks that guards and padding channels are still POISON and returns (rows, C)."""

    def __init__(self, rows, C, ld=None):
        self.rows, self.C, self.ld = int(rows), C, ld or C
        self.buf = torch.full((2 * GUARD + self.rows * self.ld,), POISON, dtype=torch.float32, device='cuda')

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * (GUARD + self.ld - self.C)

    def host(self):
        torch.cuda.synchronize()
        h = self.buf.cpu().numpy()
        assert (h[:GUARD] == POISON).all() and (h[-GUARD:] == POISON).all(), 'a guard element was written'
        body = h[GUARD:-GUARD].reshape(self.rows, self.ld)
        assert (body[:, :self.ld - self.C] == POISON).all(), 'a padding channel was written'
        return body[:, self.ld - self.C:]


def _strided(rg, N, T, C, post_relu=False):
    """A (N, T, C + PAD) float32 host buffer of random values -> (buffer, its channel slice [PAD, PAD + C) as a view)."""
    buf = rg.standard_normal((N, T, C + PAD), dtype=F32)
    if post_relu:
        np.maximum(buf, 0, out=buf)
    return buf, buf[..., PAD:]


def _slice_ptr(t):
    return t.data_ptr() + 4 * PAD


class _Checks(object):
    """The comparisons of one test.  Each is made and printed; done() fails with every one that missed, so that a test which runs
    several launches (relu 0 and 1, forward and backward, with and without skip) shows which of them are wrong, not the first."""

    def __init__(self, N, T, C):
        self.shape, self.missed = (N, T, C), []

    def equal(self, entry, got, want):
        assert got.shape == want.shape and got.dtype == want.dtype == F32
        if not np.array_equal(got, want):
            self.missed.append(c1.first_mismatch(entry, got != want, *self.shape))

    def within(self, entry, got, want, bound, tag):
        """max |got - want| <= bound * max |want|: the form of the direct tests."""
        scale = float(np.abs(want).max())
        err = float(np.abs(got - want).max()) / scale
        print('%s: max err / max |ref| = %.3g (bound %.0e)' % (tag, err, bound))
        if not err <= bound:
            self.missed.append(tag + ': ' + c1.first_mismatch(entry, ~(np.abs(got - want) <= bound * scale), *self.shape))

    def none(self, entry, bad, what):
        if bad.any():
            self.missed.append(what + ': ' + c1.first_mismatch(entry, bad, *self.shape))

    def done(self):
        if self.missed:
            pytest.fail('\n'.join(self.missed))


# ---- dc_conv1d_k5_c1_fwd ------------------------------------------------------------------------------------------------------------
def _run_c1(dclib, xd, k, scale, shift, relu, N, T, C):
    kd, sc, sh = _dev(k), _dev(scale), _dev(shift)
    y = _Out(N * T, C, C + PAD)
    dclib.dc_conv1d_k5_c1_fwd(xd.data_ptr(), kd.data_ptr(), sc.data_ptr(), sh.data_ptr(), relu, y.ptr, C + PAD, N, T, C, _st())
    return y.host().reshape(N, T, C)


@_cases('dc_conv1d_k5_c1_fwd')
def test_conv1d_k5_c1_fwd_beyond_the_grid(dclib, case):
    """Random fp32 operands (those of test_spikes_gpu.py) against float64, relu 0 and 1, at that test's 1e-4 max |reference|."""
    entry, (regime, N, T, C) = 'dc_conv1d_k5_c1_fwd', case
    ck = _Checks(N, T, C)
    rg, rs = np.random.default_rng(T + C), np.random.RandomState(T + C)
    x = rg.standard_normal((N, T), dtype=F32)
    k = (rs.randn(5, 1, C) * np.sqrt(2. / 5)).astype(F32)
    scale, shift = (1. + 0.2 * rs.randn(C)).astype(F32), (0.3 * rs.randn(C)).astype(F32)
    pre = ref.conv1d_k5(x.astype(F64)[:, :, None], k.astype(F64)) * scale.astype(F64) + shift.astype(F64)
    xd = _dev(x)
    for relu in (0, 1):
        want = np.maximum(pre, 0.) if relu else pre
        got = _run_c1(dclib, xd, k, scale, shift, relu, N, T, C)
        ck.within(entry, got, want, 1e-4, '%s %s relu=%d' % (entry, regime, relu))
    ck.done()


@_cases('dc_conv1d_k5_c1_fwd')
def test_conv1d_k5_c1_fwd_is_exact_on_integers(dclib, case):
    """x, w and shift integers in [-8, 8], scale = 1: every product is an integer of at most 64, every partial sum of the five-tap
    fmaf chain at most 5 * 64 = 320 and the affine at most 328 -- all far below 2^24, so every fmaf is exact in fp32 and the result
    must EQUAL the integer convolution.  One sample taken from the wrong place on a later trip is a wrong integer."""
    entry, (regime, N, T, C) = 'dc_conv1d_k5_c1_fwd', case
    ck = _Checks(N, T, C)
    rs = np.random.RandomState(N + C)
    x = rs.randint(-8, 9, (N, T)).astype(np.int32)
    k = rs.randint(-8, 9, (5, 1, C)).astype(np.int32)
    shift = rs.randint(-8, 9, C).astype(np.int32)
    xp = np.pad(x, ((0, 0), (2, 2)))
    pre = np.zeros((N, T, C), np.int32) + shift
    for tap in range(5):
        pre += xp[:, tap:tap + T, None] * k[tap, 0]
    assert np.abs(pre).max() <= 328 < 2 ** 24
    xd = _dev(x.astype(F32))
    for relu in (0, 1):
        want = (np.maximum(pre, 0) if relu else pre).astype(F32)
        got = _run_c1(dclib, xd, k.astype(F32), np.ones(C, F32), shift.astype(F32), relu, N, T, C)
        ck.equal(entry, got, want)
    ck.done()


# ---- dc_maxpool1d_2_fwd / _bwd ------------------------------------------------------------------------------------------------------
@_cases('dc_maxpool1d_2_fwd')
def test_maxpool1d_2_fwd_beyond_the_grid(dclib, case):
    entry, (regime, N, T, C) = 'dc_maxpool1d_2_fwd', case
    ck = _Checks(N, T, C)
    buf, x = _strided(np.random.default_rng(T), N, T, C)
    want = ref.maxpool2(x)                                                # moves values: float32 in, the same float32 out
    src, out = _dev(buf), _Out(N * (T // 2), C)
    dclib.dc_maxpool1d_2_fwd(_slice_ptr(src), C + PAD, out.ptr, N, T, C, _st())
    ck.equal(entry, out.host().reshape(N, T // 2, C), want)
    ck.done()


def _later_trip_quads(entry, N, T, C):
    """(N, rows, C4) bool: the items of a launch that are done on a later trip than the first."""
    R, C4 = c1.rows(entry, T), C // 4
    return (np.arange(N * R * C4) >= c1.CAP_ITEMS).reshape(N, R, C4)


@_cases('dc_maxpool1d_2_bwd')
def test_maxpool1d_2_bwd_beyond_the_grid(dclib, case):
    """Post-ReLU inputs: a quarter of the pairs tie at 0 (the first wins), one channel ties at 1.5.  With the skip gradient the
    result is the routed dy plus one fp32 addition, which rounds once and identically on the host; without it the routing alone."""
    entry, (regime, N, T, C) = 'dc_maxpool1d_2_bwd', case
    ck = _Checks(N, T, C)
    rg = np.random.default_rng(T)
    buf, x = _strided(rg, N, T, C, post_relu=True)
    x[:, :, 0] = 1.5
    dy = rg.standard_normal((N, T // 2, C), dtype=F32)
    sbuf = rg.random((N, T, C + PAD), dtype=F32)                          # the skip gradient: any values do, uniform ones are cheapest
    skip = sbuf[..., PAD:]
    routed = tref.pool2_bwd(x, dy).astype(F32)
    later = _later_trip_quads(entry, N, T, C)
    To, C4 = T // 2, C // 4
    ties = (x[:, 0:2 * To:2] == x[:, 1:2 * To:2]).reshape(N, To, C4, 4).any(3)
    if regime == 'cap+1':
        # its one second-trip item is the single last sample of the last trace: no pair, hence no tie, only the skip gradient
        assert later.sum() == 1 and later[N - 1, T // 2, 2] and T % 2 == 1 and not routed[N - 1, T - 1].any()
        assert ties[~later[:, :To]].any()
    else:
        n_ties = int((ties & later[:, :To]).sum())
        print('%s %s: %d of %d later-trip items hold a tie' % (entry, regime, n_ties, int(later.sum())))
        assert n_ties > 1000
    xd, dyd, sd = _dev(buf), _dev(dy), _dev(sbuf)
    ld = C + PAD
    dx = _Out(N * T, C, ld)
    dclib.dc_maxpool1d_2_bwd(dyd.data_ptr(), _slice_ptr(xd), ld, _slice_ptr(sd), ld, dx.ptr, ld, N, T, C, _st())
    ck.equal(entry, dx.host().reshape(N, T, C), routed + skip)
    del dx
    dx = _Out(N * T, C, ld)
    dclib.dc_maxpool1d_2_bwd(dyd.data_ptr(), _slice_ptr(xd), ld, None, 0, dx.ptr, ld, N, T, C, _st())
    ck.equal(entry, dx.host().reshape(N, T, C), routed)
    ck.done()


# ---- dc_upsample1d_2x_fwd / _drop_fwd / _drop_bwd -----------------------------------------------------------------------------------
def _up_fwd(dclib, xd, N, T, C, mask=None, keep=None, seed=0):
    """keep None: dc_upsample1d_2x_fwd; else dc_upsample1d_2x_drop_fwd (mask: a device tensor or None = the counter RNG).
    -> host (N, 2T, C)."""
    ld = C + PAD
    out = _Out(N * 2 * T, C, ld)
    if keep is None:
        dclib.dc_upsample1d_2x_fwd(xd.data_ptr(), out.ptr, ld, N, T, C, _st())
    else:
        dclib.dc_upsample1d_2x_drop_fwd(xd.data_ptr(), out.ptr, ld, mask.data_ptr() if mask is not None else None, keep, seed,
                                        N, T, C, _st())
    return out.host().reshape(N, 2 * T, C)


def _up_bwd(dclib, dd, N, T, C, mask, keep, seed=0):
    """dd: device (N, 2T, C + PAD), the gradient in its channel slice.  -> host (N, T, C)."""
    din = _Out(N * T, C)
    dclib.dc_upsample1d_2x_drop_bwd(_slice_ptr(dd), C + PAD, mask.data_ptr() if mask is not None else None, keep, seed, din.ptr,
                                    N, T, C, _st())
    return din.host().reshape(N, T, C)


def _pair_sum(a, N, T, C):
    """a (N, 2T, C) float32 -> a[:, 2t] + a[:, 2t + 1]: one fp32 addition per element."""
    a = a.reshape(N, T, 2, C)
    return a[:, :, 0] + a[:, :, 1]


@_cases('dc_upsample1d_2x_fwd')
def test_upsample1d_2x_fwd_beyond_the_grid(dclib, case):
    entry, (regime, N, T, C) = 'dc_upsample1d_2x_fwd', case
    ck = _Checks(N, T, C)
    x = np.random.default_rng(T).standard_normal((N, T, C), dtype=F32)
    ck.equal(entry, _up_fwd(dclib, _dev(x), N, T, C), ref.upsample2(x))
    ck.done()


@_cases('dc_upsample1d_2x_drop_fwd')
def test_upsample1d_2x_drop_keep_one_is_the_plain_kernel(dclib, case):
    """keep = 1: no mask is read, nothing is drawn, the forward is dc_upsample1d_2x_fwd bit for bit (and both are numpy's repeat),
    the backward the sum of each pair."""
    entry, (regime, N, T, C) = 'dc_upsample1d_2x_drop_fwd', case
    ck = _Checks(N, T, C)
    rg = np.random.default_rng(T + 1)
    x = rg.standard_normal((N, T, C), dtype=F32)
    xd = _dev(x)
    got = _up_fwd(dclib, xd, N, T, C, None, 1.0, SEED)
    ck.equal(entry, got, ref.upsample2(x))
    ck.equal(entry, got, _up_fwd(dclib, xd, N, T, C))
    del got
    dbuf, dout = _strided(rg, N, 2 * T, C)
    ck.equal('dc_upsample1d_2x_drop_bwd', _up_bwd(dclib, _dev(dbuf), N, T, C, None, 1.0, SEED), _pair_sum(dout, N, T, C))
    ck.done()


@pytest.mark.parametrize('keep', [0.75, 0.5])
@_cases('dc_upsample1d_2x_drop_fwd')
def test_upsample1d_2x_drop_mask_beyond_the_grid(dclib, case, keep):
    """An explicit mask.  keep = 0.75: against float64 at the direct test's 1e-6 max |reference|, zeros exactly where the mask or the
    input is zero.  keep = 0.5: the factor 2 is a power of two, products are exact and the backward's one addition rounds as the
    host's does -- equality."""
    entry, (regime, N, T, C) = 'dc_upsample1d_2x_drop_fwd', case
    ck = _Checks(N, T, C)
    rg = np.random.default_rng(T + int(8 * keep))
    x = rg.standard_normal((N, T, C), dtype=F32)
    x[:, ::7, 1] = 0.                                                     # zeros of the input itself
    mask = (rg.random((N, 2 * T, C), dtype=F32) < keep).astype(np.uint8)
    dbuf, dout = _strided(rg, N, 2 * T, C)
    md = _dev(mask)
    got = _up_fwd(dclib, _dev(x), N, T, C, md, keep, SEED)
    gin = _up_bwd(dclib, _dev(dbuf), N, T, C, md, keep, SEED)
    up = ref.upsample2(x)
    if keep == 0.5:
        fac = mask.astype(F32) * F32(2)
        ck.equal(entry, got, up * fac)
        ck.equal('dc_upsample1d_2x_drop_bwd', gin, _pair_sum(dout * fac, N, T, C))
        ck.done()
        return
    ck.within(entry, got, up.astype(F64) * mask / keep, 1e-6, '%s %s keep=%g' % (entry, regime, keep))
    ck.none(entry, (got == 0) != ((mask == 0) | (up == 0)), 'a zero that neither the mask nor the input has, or the reverse')
    want = (dout.astype(F64) * mask / keep).reshape(N, T, 2, C).sum(2)
    ck.within('dc_upsample1d_2x_drop_bwd', gin, want, 1e-6, 'dc_upsample1d_2x_drop_bwd %s keep=%g' % (regime, keep))
    ck.done()


@pytest.mark.parametrize('case', c1.CASES['dc_upsample1d_2x_drop_fwd'] + [('small',) + c1.RNG_SMALL],
                         ids=c1.case_ids('dc_upsample1d_2x_drop_fwd') + ['small-N%d-T%d-C%d' % c1.RNG_SMALL])
def test_upsample1d_2x_drop_rng_is_the_oracles_hash(dclib, case):
    """mask = NULL: the kept positions of an input of ones are oracle.unet_numpy.hash_keep_mask over the DENSE up-sampled tensor,
    element (n * 2T + u) * C + c, whatever the sample stride; the backward of ones is the pairwise sum of the same mask.  The
    small shape runs one workgroup: a convention mismatch between the 1-D kernels and the oracle's hash shows there as such."""
    regime, N, T, C = case
    ck = _Checks(N, T, C)
    keep = 0.75
    m = on.hash_keep_mask(SEED, N * 2 * T * C, keep).reshape(N, 2 * T, C)
    assert 0.74 < m.mean() < 0.76 or regime == 'small'
    want = m.astype(F32) * (F32(1) / F32(keep))                                      # 1 * fl(1 / keep), or 0
    assert want.dtype == F32
    got = _up_fwd(dclib, _dev(np.ones((N, T, C), F32)), N, T, C, None, keep, SEED)
    ck.equal('dc_upsample1d_2x_drop_fwd', got, want)
    dbuf, dout = _strided(np.random.default_rng(T), N, 2 * T, C)
    dout[...] = 1.
    gin = _up_bwd(dclib, _dev(dbuf), N, T, C, None, keep, SEED)
    ck.equal('dc_upsample1d_2x_drop_bwd', gin, _pair_sum(want, N, T, C))
    if regime == 'small':                                                 # another seed, another mask
        other = _up_fwd(dclib, _dev(np.ones((N, T, C), F32)), N, T, C, None, keep, SEED + 1)
        assert np.array_equal(other != 0, on.hash_keep_mask(SEED + 1, N * 2 * T * C, keep).reshape(N, 2 * T, C) != 0)
        assert not np.array_equal(other, got)
    ck.done()


# ---- the engine: capped launches on their second and third trips, uncapped ones on tens of thousands of workgroups ------------------
@pytest.fixture(scope='module')
def engine_run(dclib):
    """One forward of 1101 traces of 4096 samples at nfb 4, and the same traces in consecutive batches of 256, whose capped launches
    all stay on their first trip (tests/test_caps1d.py).  -> (weights, traces, whole (B, T), batched (B, T)), host arrays."""
    from deep_calcium_amd import UNet1DEngine
    e = c1.ENGINE
    w = ref.make_model(e['nfb'], e['model_seed'])
    x = ref.make_traces(e['B'], e['T'], e['trace_seed'])
    eng = UNet1DEngine(w, e['nfb'], e['margin'])
    xd = _dev(x)
    t0 = time.time()
    whole = eng.forward(xd).cpu().numpy()
    parts = np.concatenate([eng.forward(xd[a:a + e['sub']]).cpu().numpy() for a in range(0, e['B'], e['sub'])])
    print('UNet1DEngine: %d traces at once and in batches of %d: %.2f s' % (e['B'], e['sub'], time.time() - t0))
    del eng, xd                                                           # 1.1 GB of engine buffers
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return w, x, whole, parts


def test_engine_forward_beyond_the_grid_equals_its_batches(engine_run):
    """The batching invariance deep_calcium_amd/spikes.py documents, where one side of it runs every capped launch into a later trip."""
    w, x, whole, parts = engine_run
    assert whole.shape == parts.shape == x.shape and whole.dtype == F32
    differ = np.flatnonzero((whole != parts).any(1))
    print('UNet1DEngine.forward %r: %d traces differ from their batch of %d' % (x.shape, differ.size, c1.ENGINE['sub']))
    assert differ.size == 0, 'the first trace that differs is %d (pooling takes its second trip from trace 1024, the first layer from 512)' % differ[0]


def test_engine_forward_beyond_the_grid_equals_the_oracle(engine_run):
    w, x, whole, parts = engine_run
    rows = list(c1.ENGINE['oracle_traces'])
    want = ref.forward(w, x[rows], c1.ENGINE['margin'])
    assert ((want > 0.05) & (want < 0.95)).mean() >= 0.5                  # the oracle stays informative
    err = np.abs(whole[rows] - want).max(1)
    print('UNet1DEngine.forward traces %r: max |p - oracle| = %r' % (rows, ['%.3g' % v for v in err]))
    assert err.max() <= 1e-4
