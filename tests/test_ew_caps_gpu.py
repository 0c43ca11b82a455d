"""Every capped-grid kernel of csrc/elementwise.hip past its cap (DESIGN.md 4f-caps-2d has the table): the BatchNorm passes clamp their
grid at 1 280 workgroups, pooling / Adam / fill / merge at 2 048 or 4 096 workgroups of 256 items, dc_crop_augment and
dc_round_window_u8 at 64 and 256 workgroups per image, and a workgroup strides over the rest.  The other modules compare these
kernels with an independent reference on the first trip only; here every entry point runs a launch whose later trips carry real
work (tests/_ewcaps.py has the shapes, tests/test_ew_caps.py checks on the CPU that each lands in the regime claimed for it).

Oracles: the float64 functions of oracle/unet_numpy.py, or numpy written here.  Every output buffer starts as NaN (0xA5 for uint8)
and has GUARD elements on both sides that must stay untouched.  Tolerances are those of the small-shape tests of the same entry
point (tests/test_hip_ops.py, tests/test_glue_ops_gpu.py); sums are held to n u sum|x| (an fp32 sum of n terms in any order) and,
on integer-valued data whose fp32 sums are exact, to equality: a pixel lost or taken twice on a later trip is then a wrong count.

The ReLU gate [y > 0] is discontinuous: a pre-activation within fp32 rounding of 0 could fall on either side on the device.  The
float64 pre-activations of the random inputs are therefore kept GATE_MARGIN away from 0 (the few elements inside are moved), far
more than the 2e-6 the fp32 evaluation of z * sc + sh can be off at |z| < 10."""
import numpy as np
import pytest

from oracle import unet_numpy as on

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _ewcaps as ec                  # noqa: E402

U = 2.0 ** -24                        # unit round-off of fp32
GUARD = 8
GATE_MARGIN = 1e-4
SEED = 0xA5A5A5A5DEADBEEF
F32, F64 = np.float32, np.float64


@pytest.fixture(autouse=True)
def _release_device_memory():
    """The buffers here reach a few hundred MB: hand them back, so that one test's cached blocks do not add to the next one's."""
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class _Out(object):
    """n output elements inside a buffer pre-filled with NaN (0xA5 for uint8), GUARD elements on both sides.  at(k): the address
    of element k; get() synchronises and checks that no guard element changed."""

    def __init__(self, n, dtype=torch.float32):
        self.n, self.fp = int(n), dtype.is_floating_point
        self.buf = torch.full((self.n + 2 * GUARD,), float('nan') if self.fp else 0xA5, dtype=dtype, device='cuda')

    def at(self, k=0):
        return self.buf.data_ptr() + (GUARD + k) * self.buf.element_size()

    @property
    def ptr(self):
        return self.at(0)

    def untouched(self, t):
        return bool(torch.isnan(t).all()) if self.fp else bool((t == 0xA5).all())

    def get(self, *shape):
        torch.cuda.synchronize()
        assert self.untouched(self.buf[:GUARD]) and self.untouched(self.buf[GUARD + self.n:]), 'a guard element was written'
        return self.buf[GUARD:GUARD + self.n].view(*shape)

    def host(self, *shape):
        return self.get(*shape).cpu().numpy()


def _strided_in(dense, ld):
    """dense (P, C) as the LAST C columns of a (P, ld) device buffer of other values; -> (buffer, address of the first element)."""
    P, C = dense.shape
    buf = torch.randn(P, ld, device='cuda') * 3
    buf[:, ld - C:] = dev(dense)
    return buf, buf.data_ptr() + 4 * (ld - C)


def _keep_gates_clear(z, pre):
    """Move the elements of z (float32, in place) whose float64 pre-activation pre(z) lies within GATE_MARGIN of 0; -> pre(z)."""
    for _ in range(8):
        y = pre(z)
        near = np.abs(y) < GATE_MARGIN
        if not near.any():
            return y
        z[near.reshape(z.shape)] += F32(0.01)
    raise AssertionError('pre-activations stay near 0')


def _drop(rs, kind, shape, n_hash):
    """(keep, mask uint8 of `shape`, whether the device draws it): 'rng' = the counter hash over the first n_hash dense elements."""
    n = int(np.prod(shape))
    if kind == 'none':
        return 1.0, np.ones(shape, np.uint8), False
    keep = 0.75
    mask = (rs.random_sample(n) < keep).astype(np.uint8)
    if kind == 'rng':
        mask[:n_hash] = on.hash_keep_mask(SEED, n_hash, keep)
    return keep, mask.reshape(shape), kind == 'rng'


def _within(got, ref, bound, tag):
    got, ref = np.asarray(got, F64), np.asarray(ref, F64)
    worst = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max())
    print('%s: worst |got - ref| / bound = %.3g' % (tag, worst))
    assert np.isfinite(got).all() and (np.abs(got - ref) <= bound).all(), tag


# ---- 1. the BatchNorm passes: 1 280 workgroups of PPB = 1024 / C pixel lanes -------------------------------------------------------
class _BnCase(object):
    """One (regime, C, dropout, stride) of _ewcaps.BN_CASES.  The launches see the first P pixels of a batch of T = P + BN_EXTRA
    whose statistics are the whole batch's (what a data-parallel shard sees); the float64 oracle is evaluated once."""

    def __init__(self, regime, C, drop, ld):
        self.regime, self.C, self.ld, self.off = regime, C, ld, ld - C
        P = self.P = ec.bn_pixels(regime, C)
        T = self.T = P + ec.BN_EXTRA
        rs = np.random.RandomState(1000 * regime + C)
        z = (rs.standard_normal((T, C)) * 1.7 + 0.4).astype(F32)
        gamma, beta = rs.uniform(0.5, 1.5, C).astype(F32), rs.uniform(-0.5, 0.5, C).astype(F32)
        g64, b64 = gamma.astype(F64), beta.astype(F64)
        da = rs.standard_normal((T, C)).astype(F32)
        self.keep, mask, self.rng = _drop(rs, drop, (T, C), P * C)
        kept = {}

        def pre(v):
            kept['y'], kept['cache'] = on.bn_train_fwd(v.astype(F64).reshape(1, 1, T, C), g64, b64)
            return kept['y']
        _keep_gates_clear(z, pre)                                            # the statistics are those of the z that is kept
        y, cache = kept['y'], kept['cache']
        fac = mask / self.keep if self.keep < 1 else 1.0
        self.a_ref = (np.maximum(y, 0) * fac)[0, 0, :P]
        dy = da.astype(F64) * fac * (y > 0)                                  # (1, 1, T, C)
        xhat, inv = cache[0], cache[1]
        self.dz_all, self.dg_all, self.db_all = on.bn_train_bwd(dy, g64, cache)          # count = T
        self.dz_P, self.dg_P, self.db_P = on.bn_train_bwd(dy[:, :, :P], g64, (xhat[:, :, :P], inv))
        self.dz_all, self.dz_P = self.dz_all[0, 0, :P], self.dz_P[0, 0]
        self.sabs_db, self.sabs_dg = np.abs(dy[0, 0, :P]).sum(0), np.abs(dy * xhat)[0, 0, :P].sum(0)
        # max |dy| per channel as the device forms dy: one fp32 product with fl(1 / keep), then the gate
        f32 = mask[:P].astype(F32) * (F32(1) / F32(self.keep)) if self.keep < 1 else F32(1)
        self.amax_dy = np.abs(da[:P] * f32 * (y[0, 0, :P] > 0)).max(0).astype(F32)
        self.abound = (np.abs(g64) * np.sqrt(float(T)) + np.abs(b64)) / self.keep
        self.zd, self.gd, self.bd = dev(z[:P]), dev(gamma), dev(beta)
        self.mean, self.invstd = dev(cache[2].astype(F32)), dev(cache[1].astype(F32))
        self.dabuf, self.da_ptr = _strided_in(da[:P], ld)
        self.maskd = dev(mask[:P]) if (self.keep < 1 and not self.rng) else None
        self.mptr = self.maskd.data_ptr() if self.maskd is not None else None
        self.seed = SEED if self.rng else 0

    def bwd_args(self):
        return (self.da_ptr, self.ld, self.zd.data_ptr(), self.mean.data_ptr(), self.invstd.data_ptr(), self.gd.data_ptr(),
                self.bd.data_ptr(), self.mptr, self.keep, self.seed)


@pytest.fixture(scope='module', params=ec.BN_CASES, ids=lambda c: 'r%d-C%d-%s-ld%d' % c)
def bn(request):
    case = _BnCase(*request.param)
    yield case
    case.__dict__.clear()
    torch.cuda.empty_cache()


def test_bn_relu_drop_fwd_beyond_the_grid(dclib, bn):
    """dc_bn_relu_drop_fwd against float64 BN + ReLU + dropout at the 2e-5 of test_batchnorm_relu_dropout_fwd_bwd, strided into a
    wider buffer; the bound output (written once, by workgroup 0) is the one a one-workgroup launch writes."""
    L, P, C, ld = dclib, bn.P, bn.C, bn.ld
    assert ec.bn_trips(P, C)[0] >= 2
    out, ab = _Out(P * ld), _Out(C)
    head = (bn.mean.data_ptr(), bn.invstd.data_ptr(), bn.gd.data_ptr(), bn.bd.data_ptr(), bn.mptr, bn.keep, bn.seed)
    L.dc_bn_relu_drop_fwd(bn.zd.data_ptr(), *head, out.at(bn.off), ld, P, C, float(bn.T), ab.ptr, None)
    o = out.get(P, ld)
    assert out.untouched(o[:, :bn.off])
    err = np.abs(o[:, bn.off:].cpu().numpy() - bn.a_ref).max()
    print('dc_bn_relu_drop_fwd P=%d C=%d: max|a - ref| = %.3e' % (P, C, err))
    assert err < 2e-5
    small, ab1 = _Out(ec.ppb(C) * ld), _Out(C)
    L.dc_bn_relu_drop_fwd(bn.zd.data_ptr(), *head, small.at(bn.off), ld, ec.ppb(C), C, float(bn.T), ab1.ptr, None)
    assert torch.equal(ab.get(C).view(torch.int32), ab1.get(C).view(torch.int32))
    assert np.allclose(ab.host(C), bn.abound, rtol=1e-6, atol=0)
    assert np.abs(small.host(ec.ppb(C), ld)[:, bn.off:] - bn.a_ref[:ec.ppb(C)]).max() < 2e-5


def _check_apply(bn, dz, dbp, absmax, dz_ref, blocks, what):
    P, C = bn.P, bn.C
    dzh = dz.host(P, C)
    err = np.abs(dzh - dz_ref).max()
    print('%s P=%d C=%d: max|dz - ref| = %.3e (scale %.3e)' % (what, P, C, err, np.abs(dz_ref).max()))
    assert err < 3e-5 * max(np.abs(dz_ref).max(), 1)
    d64 = dzh.astype(F64)
    _within(dbp.host(blocks, C).astype(F64).sum(0), d64.sum(0), P * U * np.abs(d64).sum(0), what + ' dbias_partial')
    assert absmax.host(blocks).max() == np.abs(dzh).max()


def test_bn_bwd_reduce_and_apply_beyond_the_grid(dclib, bn):
    """dc_bn_bwd_reduce -> dc_bn_bwd_finalize -> dc_bn_bwd_apply, as a step chains them, against float64 bn_train_bwd."""
    L, P, C = dclib, bn.P, bn.C
    blocks = L.dc_bn_bwd_blocks(P, C)
    assert blocks == ec.K_MAX_BLOCKS == ec.bn_blocks(P, C) and ec.sweep_trips(P, C) == ec.BN_REGIMES[bn.regime][0]
    part, amx, dg, db = _Out(blocks * C * 2), _Out(blocks * C), _Out(C), _Out(C)
    L.dc_bn_bwd_reduce(*bn.bwd_args(), part.ptr, amx.ptr, P, C, None)
    L.dc_bn_bwd_finalize(part.ptr, blocks, C, dg.ptr, db.ptr, None)
    dz, dbp, absmax = _Out(P * C), _Out(blocks * C), _Out(blocks)
    L.dc_bn_bwd_apply(*bn.bwd_args(), dg.ptr, db.ptr, dz.ptr, dbp.ptr, absmax.ptr, P, C, None)
    # the terms themselves carry a few u each (fl(1 / keep), xhat): nothing beside the n >= 1 923 of the bound
    _within(db.host(C), bn.db_P, P * U * bn.sabs_db, 'dbeta')
    _within(dg.host(C), bn.dg_P, P * U * bn.sabs_dg, 'dgamma')
    assert np.array_equal(amx.host(blocks, C).max(0), bn.amax_dy)
    _check_apply(bn, dz, dbp, absmax, bn.dz_P, blocks, 'dc_bn_bwd_apply')


def test_bn_bwd_apply_count_beyond_the_grid(dclib, bn):
    """dc_bn_bwd_apply_count as a data-parallel shard calls it: count = the whole batch's pixels > pixels, the whole batch's sums."""
    L, P, C = dclib, bn.P, bn.C
    blocks = L.dc_bn_bwd_blocks(P, C)
    assert blocks == ec.K_MAX_BLOCKS and bn.T > P
    dg, db = dev(bn.dg_all.astype(F32)), dev(bn.db_all.astype(F32))
    dz, dbp, absmax = _Out(P * C), _Out(blocks * C), _Out(blocks)
    L.dc_bn_bwd_apply_count(*bn.bwd_args(), dg.data_ptr(), db.data_ptr(), dz.ptr, dbp.ptr, absmax.ptr, P, float(bn.T), C, None)
    _check_apply(bn, dz, dbp, absmax, bn.dz_all, blocks, 'dc_bn_bwd_apply_count')


@pytest.mark.parametrize('regime,C', [(c[0], c[1]) for c in ec.BN_CASES])
def test_bn_bwd_reduce_counts_every_pixel_once(dclib, regime, C):
    """Integer-valued z and da, mean 0, invstd 1, gamma 1, beta 1/2: dy = da [z >= 0] and dy * xhat = dy z are small integers, every
    fp32 partial sum is exact, and the finalized sums must EQUAL the integer sums -- one pixel lost or taken twice is a miss."""
    L, P = dclib, ec.bn_pixels(regime, C)
    rs = np.random.RandomState(7 * regime + C)
    z, da = rs.randint(-3, 4, size=(P, C)), rs.randint(-4, 5, size=(P, C))
    da[P - 1] = 4 * np.where(np.arange(C) % 2, 1, -1)                       # the last pixel holds every channel's max |dy| ...
    z[P - 1] = 2
    da[:P - 1][np.abs(da[:P - 1]) == 4] = 3                                 # ... alone
    dy = da * (z >= 0)
    s1, s2 = dy.sum(0), (dy * z).sum(0)
    assert max(np.abs(dy).sum(0).max(), np.abs(dy * z).sum(0).max()) < 2 ** 24
    v = {k: dev(np.full(C, x, F32)) for k, x in (('mean', 0), ('invstd', 1), ('gamma', 1), ('beta', 0.5))}
    ld = C + 4
    zd = dev(z.astype(F32))
    dabuf, da_ptr = _strided_in(da.astype(F32), ld)
    blocks = L.dc_bn_bwd_blocks(P, C)
    part, amx, dg, db = _Out(blocks * C * 2), _Out(blocks * C), _Out(C), _Out(C)
    L.dc_bn_bwd_reduce(da_ptr, ld, zd.data_ptr(), v['mean'].data_ptr(), v['invstd'].data_ptr(), v['gamma'].data_ptr(),
                       v['beta'].data_ptr(), None, 1.0, 0, part.ptr, amx.ptr, P, C, None)
    L.dc_bn_bwd_finalize(part.ptr, blocks, C, dg.ptr, db.ptr, None)
    assert np.array_equal(db.host(C), s1.astype(F32)) and np.array_equal(dg.host(C), s2.astype(F32))
    a = amx.host(blocks, C)
    assert np.array_equal(a.max(0), np.full(C, 4, F32)) and (a == 4).sum() == C


# ---- 2. dc_bn_relu_drop_pool_fwd: 1 280 workgroups of 256 windows x 4 channels -------------------------------------------------------
@pytest.mark.parametrize('shape,drop', list(zip(ec.POOL_FUSED_SHAPES, ('rng', 'mask', 'none'))), ids=lambda v: str(v).replace(' ', ''))
def test_bn_relu_drop_pool_fwd_beyond_the_grid(dclib, shape, drop):
    """Activation (strided into a wider buffer) against float64 at 2e-5; pooled values and argmax are the float32 oracle's on the
    activation the kernel wrote, exactly."""
    L = dclib
    N, H, W, C = shape
    pix, items, ld = N * H * W, ec.pool_items(*shape), C + 8
    assert items > ec.K_MAX_BLOCKS * ec.THREADS
    rs = np.random.RandomState(H + C)
    z = (rs.standard_normal(shape) * 1.7 + 0.4).astype(F32)
    gamma, beta = rs.uniform(0.5, 1.5, C).astype(F32), rs.uniform(-0.5, 0.5, C).astype(F32)
    keep, mask, rng = _drop(rs, drop, shape, pix * C)
    y, cache = on.bn_train_fwd(z.astype(F64), gamma.astype(F64), beta.astype(F64))
    a_ref = np.maximum(y, 0) * (mask / keep if keep < 1 else 1.0)
    del y
    zd, maskd = dev(z), dev(mask)
    v = [dev(a) for a in (cache[2].astype(F32), cache[1].astype(F32), gamma, beta)]
    out, pooled, idx, ab = _Out(pix * ld), _Out(items * 4), _Out(items * 4, torch.uint8), _Out(C)
    L.dc_bn_relu_drop_pool_fwd(zd.data_ptr(), v[0].data_ptr(), v[1].data_ptr(), v[2].data_ptr(), v[3].data_ptr(),
                               maskd.data_ptr() if (keep < 1 and not rng) else None, keep, SEED if rng else 0, out.at(8), ld,
                               pooled.ptr, idx.ptr, N, H, W, C, float(pix), ab.ptr, None)
    o = out.get(pix, ld)
    assert out.untouched(o[:, :8])
    act = o[:, 8:].contiguous().cpu().numpy().reshape(shape)
    err = np.abs(act - a_ref).max()
    print('dc_bn_relu_drop_pool_fwd %s: max|a - ref| = %.3e' % (shape, err))
    assert err < 2e-5
    p_ref, i_ref = on.maxpool2x2_fwd(act)
    assert p_ref.dtype == F32 and (i_ref > 0).any() and (p_ref == 0).any()          # ties at 0: the first one wins
    assert np.array_equal(pooled.host(N, H // 2, W // 2, C), p_ref)
    assert np.array_equal(idx.host(N, H // 2, W // 2, C), i_ref)
    assert np.allclose(ab.host(C), (np.abs(gamma.astype(F64)) * np.sqrt(float(pix)) + np.abs(beta)) / keep, rtol=1e-6, atol=0)


# ---- 3. dc_maxpool2x2_fwd / _bwd: 4 096 workgroups ---------------------------------------------------------------------------------
class _PoolCase(object):
    def __init__(self):
        N, H, W, C = self.shape = ec.POOL_SHAPE
        rs = np.random.RandomState(3)
        self.x = np.maximum(rs.standard_normal(self.shape), 0).astype(F32)          # post-ReLU: ties at 0
        self.x[N - 1, H - 4:, W - 4:] = 1.5                                         # all-equal windows on the second trip
        self.p_ref, self.i_ref = on.maxpool2x2_fwd(self.x)
        self.dy = rs.standard_normal(self.p_ref.shape).astype(F32)
        self.routed = on.maxpool2x2_bwd(self.dy, self.i_ref)
        self.skip = rs.standard_normal(self.shape).astype(F32)


@pytest.fixture(scope='module')
def pool():
    case = _PoolCase()
    yield case
    case.__dict__.clear()


def test_maxpool_fwd_beyond_the_grid(dclib, pool):
    N, H, W, C = pool.shape
    items, ld = ec.pool_items(*pool.shape), C + 4
    assert ec.flat_trips(items, ec.CAP_4096) == (2, 1) and items % ec.THREADS
    xbuf, x_ptr = _strided_in(pool.x.reshape(-1, C), ld)
    out, idx = _Out(items * 4), _Out(items * 4, torch.uint8)
    dclib.dc_maxpool2x2_fwd(x_ptr, ld, out.ptr, idx.ptr, N, H, W, C, None)
    assert torch.equal(out.get(*pool.p_ref.shape).view(torch.int32), dev(pool.p_ref).view(torch.int32))
    assert torch.equal(idx.get(*pool.i_ref.shape), dev(pool.i_ref))
    assert (pool.i_ref[N - 1, -2:, -2:] == 0).all() and (pool.i_ref > 0).any()


@pytest.mark.parametrize('with_skip', [True, False])
def test_maxpool_bwd_beyond_the_grid(dclib, pool, with_skip):
    """dx = the routed gradient (+ the skip gradient, one fp32 addition), equal to the float32 oracle's value for value (the oracle
    routes -0 where the kernel, adding to +0, writes +0)."""
    N, H, W, C = pool.shape
    ld = C + 8
    dyd, idd = dev(pool.dy), dev(pool.i_ref)
    dx = _Out(N * H * W * C)
    if with_skip:
        skbuf, sk_ptr = _strided_in(pool.skip.reshape(-1, C), ld)
        want = pool.routed + pool.skip
    else:
        sk_ptr, ld, want = None, 0, pool.routed
    dclib.dc_maxpool2x2_bwd(dyd.data_ptr(), idd.data_ptr(), sk_ptr, ld, dx.ptr, N, H, W, C, None)
    assert want.dtype == F32 and torch.equal(dx.get(N, H, W, C), dev(want))


# ---- 4. dc_maxpool2x2_bwd_bnred: 2 048 workgroups, sums carried across the trips -----------------------------------------------------
def _bnred_launch(L, shape, dy, idx, skip, ld, z, vec, mask, keep, seed):
    """-> (dx (pix, C) float32, dgamma, dbeta float32 (C,), per-channel max over the rows of amax_partial)"""
    N, H, W, C = shape
    P = L.dc_maxpool2x2_bwd_blocks(N, H, W, C)
    assert P == ec.CAP_2048 == ec.flat_blocks(ec.pool_items(*shape), ec.CAP_2048)
    dyd, idd, zd = dev(dy), dev(idx), dev(z)
    skbuf, sk_ptr = _strided_in(skip.reshape(-1, C), ld)
    vd = [dev(a) for a in vec]
    md = dev(mask) if mask is not None else None
    dx, part, amx, dg, db = _Out(N * H * W * C), _Out(P * C * 2), _Out(P * C), _Out(C), _Out(C)
    L.dc_maxpool2x2_bwd_bnred(dyd.data_ptr(), idd.data_ptr(), sk_ptr, ld, dx.ptr, zd.data_ptr(), vd[0].data_ptr(), vd[1].data_ptr(),
                              vd[2].data_ptr(), vd[3].data_ptr(), md.data_ptr() if md is not None else None, keep, seed, part.ptr,
                              amx.ptr, N, H, W, C, None)
    L.dc_bn_bwd_finalize(part.ptr, P, C, dg.ptr, db.ptr, None)
    return dx.host(N * H * W, C), dg.host(C), db.host(C), amx.host(P, C).max(0)


@pytest.mark.parametrize('shape,drop', list(zip(ec.POOL_BNRED_SHAPES, ('mask', 'rng'))), ids=lambda v: str(v).replace(' ', ''))
def test_maxpool_bwd_bnred_beyond_the_grid(dclib, shape, drop):
    """dx equal to the float32 oracle; the BatchNorm-backward sums and the per-channel max |dy| against float64 / float32 numpy of
    the dx the kernel wrote.  C / 4 = 2 and 64 channel quads: a thread that took another quad on a later trip would add to
    another channel's sums.  Then the same launch on integer-valued data (keep = 1/2: a factor of 2), where the sums are exact."""
    L = dclib
    N, H, W, C = shape
    pix, ld = N * H * W, C + 8
    rs = np.random.RandomState(C)
    z = (rs.standard_normal((pix, C)) * 1.7 + 0.4).astype(F32)
    gamma, beta = rs.uniform(0.5, 1.5, C).astype(F32), rs.uniform(-0.5, 0.5, C).astype(F32)
    z64 = z.astype(F64)
    mean, invstd = z64.mean(0).astype(F32), (1 / np.sqrt(z64.var(0) + 1e-3)).astype(F32)
    del z64
    sc = gamma * invstd                                                         # dc_bn_affine's own fp32 constants
    sh = (beta.astype(F64) - mean.astype(F64) * sc.astype(F64)).astype(F32)
    pre = lambda v: v.astype(F64) * sc.astype(F64) + sh.astype(F64)             # noqa: E731
    gate = _keep_gates_clear(z, pre) > 0
    dy = rs.standard_normal((N, H // 2, W // 2, C)).astype(F32)
    idx = rs.randint(0, 4, dy.shape).astype(np.uint8)
    skip = (rs.standard_normal((pix, C)) + 0.25 * (1 + np.arange(C) % 5)).astype(F32)      # channel-dependent means
    keep, mask, rng = _drop(rs, drop, (pix, C), pix * C)
    dx, dg, db, amax = _bnred_launch(L, shape, dy, idx, skip, ld, z, (mean, invstd, gamma, beta), None if rng else mask, keep,
                                     SEED if rng else 0)
    want = on.maxpool2x2_bwd(dy, idx).reshape(pix, C) + skip
    assert want.dtype == F32 and np.array_equal(dx, want)
    d64 = dx.astype(F64) * gate * (mask / keep)
    xhat = (z.astype(F64) - mean.astype(F64)) * invstd.astype(F64)
    _within(db, d64.sum(0), pix * U * np.abs(d64).sum(0), 'dbeta')
    _within(dg, (d64 * xhat).sum(0), pix * U * np.abs(d64 * xhat).sum(0), 'dgamma')
    d32 = dx * (mask.astype(F32) * (F32(1) / F32(keep))) * gate
    assert d32.dtype == F32 and np.array_equal(amax, np.abs(d32).max(0))
    del d64, xhat, d32, want
    # integers: dy = (routed + skip) * 2 mask * [z >= 0], xhat = z
    zi, dyi, ski = rs.randint(-3, 4, size=(pix, C)), rs.randint(-4, 5, size=dy.shape), rs.randint(-4, 5, size=(pix, C))
    mi = (rs.random_sample((pix, C)) < 0.5).astype(np.uint8)
    consts = tuple(np.full(C, x, F32) for x in (0, 1, 1, 0.5))
    dx, dg, db, amax = _bnred_launch(L, shape, dyi.astype(F32), idx, ski.astype(F32), ld, zi.astype(F32), consts, mi, 0.5, 0)
    wi = on.maxpool2x2_bwd(dyi, idx).reshape(pix, C) + ski
    di = wi * 2 * mi * (zi >= 0)
    # a workgroup adds 3 072 terms of 48 at most, the finalize adds its rows in double: exact as long as the total fits fp32
    assert max(np.abs(di.sum(0)).max(), np.abs((di * zi).sum(0)).max()) < 2 ** 24
    assert np.array_equal(dx, wi.astype(F32))
    assert np.array_equal(db, di.sum(0).astype(F32)) and np.array_equal(dg, (di * zi).sum(0).astype(F32))
    assert np.array_equal(amax, np.abs(di).max(0).astype(F32))


# ---- 5. dc_adam_step_flat: 4 096 workgroups x 256 threads x 4 parameters --------------------------------------------------------------
class _AdamCase(object):
    """Three Keras-form steps in float64 on the longest n; the kernel's arithmetic is elementwise, so a shorter n is a prefix.  The
    oracle gets b1, b2 and eps as the fp32 values the kernel receives."""
    GSCALE = (1.0, float(F32(1.0 / 3.0)), 1.0)

    def __init__(self):
        n = max(ec.ADAM_N)
        rs = np.random.RandomState(0)
        self.p0, self.g = rs.standard_normal(n).astype(F32), (rs.standard_normal(n) * 1e-3).astype(F32)
        self.g[:3] = 1.0
        self.g[-7:] = -1.0
        b1, b2, eps = float(F32(0.9)), float(F32(0.999)), float(F32(1e-8))
        p, m, v = self.p0.astype(F64), np.zeros(n), np.zeros(n)
        env = np.zeros(n)                                                   # b1 env + (1 - b1) |g|: what m's roundings are relative to
        self.lr_t = []
        for it, gs in enumerate(self.GSCALE):
            self.lr_t.append(float(0.002 * np.sqrt(1 - b2 ** (it + 1)) / (1 - b1 ** (it + 1))))
            g64 = self.g.astype(F64) * gs
            env = b1 * env + (1 - b1) * np.abs(g64)
            p, m, v = on.adam_keras(p, g64, m, v, it, lr=0.002, b1=b1, b2=b2, eps=eps)
        self.p, self.m, self.v, self.env = p, m, v, env


@pytest.fixture(scope='module')
def adam():
    case = _AdamCase()
    yield case
    case.__dict__.clear()


@pytest.mark.parametrize('n', ec.ADAM_N)
def test_adam_beyond_the_grid(dclib, adam, n):
    """p at the 1e-6 of test_adam_keras_form; m and v to their rounding counts: a step rounds m at most 4 times (g * gscale, two
    products, one sum: 4 u of b1 |m| + (1 - b1) |g|) and v at most 7 times (g * gscale enters twice), and carries the earlier
    steps' error on."""
    assert ec.flat_trips(n // 4, ec.CAP_4096) == (3, 2) and n % 4 in (2, 3)
    bufs = [_Out(n) for _ in range(4)]
    p, g, m, v = [b.buf[GUARD:GUARD + n] for b in bufs]
    p.copy_(dev(adam.p0[:n])); g.copy_(dev(adam.g[:n])); m.zero_(); v.zero_()
    for it, gs in enumerate(adam.GSCALE):
        dclib.dc_adam_step_flat(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, n, adam.lr_t[it], 0.9, 0.999, 1e-8, gs, None)
    ph, gh, mh, vh = [b.host(n) for b in bufs]
    steps = len(adam.GSCALE)
    assert np.array_equal(gh, adam.g[:n])
    err = np.abs(ph - adam.p[:n]).max()
    print('dc_adam_step_flat n=%d: max|p - ref| = %.3e' % (n, err))
    assert err < 1e-6
    _within(mh, adam.m[:n], 4 * U * steps * adam.env[:n], 'm')
    _within(vh, adam.v[:n], 7 * U * steps * adam.v[:n], 'v')
    # a parameter the kernel skipped would show: three sign-like steps of lr move all but the few with |g| near eps
    assert (np.abs(adam.p[:n] - adam.p0[:n]) > 1e-3).mean() > 0.999


# ---- 6. dc_fill: 2 048 workgroups ----------------------------------------------------------------------------------------------------
def test_fill_beyond_the_grid(dclib):
    n = ec.FILL_N
    assert ec.flat_trips(n, ec.CAP_2048) == (2, 1)
    out = _Out(n)
    dclib.dc_fill(out.ptr, n, -3.25, None)
    assert bool((out.get(n) == -3.25).all())


# ---- 7. dc_tta_merge: 4 096 workgroups -----------------------------------------------------------------------------------------------
def test_tta_merge_beyond_the_grid(dclib):
    """mean_out == float32 of the float64 table-order sum, bit for bit, mask == m > threshold, with pixels on the threshold and one
    fp32 ulp either side among the second trip's (tests/test_glue_ops_gpu.py test_tta_merge_mean_and_threshold, vectorised)."""
    H, W, hs, ws, K = (ec.TTA[k] for k in ('H', 'W', 'hs', 'ws', 'K'))
    threshold = 0.5
    rs = np.random.RandomState(K)
    ident = np.arange(H * W, dtype=np.int32).reshape(H, W)
    maps = np.stack([np.rot90(ident, k).ravel() for k in range(K)]).astype(np.int32)
    inv = np.stack([np.argsort(m, kind='stable') for m in maps]).astype(np.int32)
    target = rs.random_sample((K, H, W)).astype(F32)
    t32 = F32(threshold)
    on_thr = [t32, np.nextafter(t32, F32(0)), np.nextafter(t32, F32(1))]
    first = ec.CAP_4096 * ec.THREADS                                          # the first cropped pixel of the second trip
    spots = [divmod(i, ws) for i in (first, first + 1, hs * ws - 1, first + 5000, first - 1, 0)]
    for i, (y, x) in enumerate(spots):
        target[:, y, x] = on_thr[i % 3]
    preds = np.stack([target[k].ravel()[maps[k]] for k in range(K)])
    acc = np.zeros(H * W, F64)
    for k in range(K):
        acc += preds[k][inv[k]].astype(F64) / K
    m_ref = acc.reshape(H, W)[:hs, :ws]
    assert np.array_equal(preds[1][inv[1]].reshape(H, W), target[1])
    pd, invd = dev(preds), dev(inv)
    for with_mean in (True, False):
        mask, mean = _Out(hs * ws, torch.uint8), _Out(hs * ws)
        dclib.dc_tta_merge(pd.data_ptr(), invd.data_ptr(), K, H, W, hs, ws, threshold, mask.ptr, mean.ptr if with_mean else None, None)
        mk = mask.host(hs, ws)
        assert np.array_equal(mk, (m_ref > threshold).astype(np.uint8))
        mn = mean.get(hs, ws)
        if with_mean:
            assert torch.equal(mn.view(torch.int32), dev(m_ref.astype(F32)).view(torch.int32))
        else:
            assert mean.untouched(mn)
    for i, (y, x) in enumerate(spots):
        assert m_ref[y, x] == float(on_thr[i % 3]) and mk[y, x] == (1 if on_thr[i % 3] > t32 else 0)


# ---- 8. dc_crop_augment: 64 workgroups per image, 4 pixels of a row per thread ---------------------------------------------------------
@pytest.mark.parametrize('hw', ec.CROP_HW)
def test_crop_augment_beyond_the_grid(dclib, hw):
    Hs, Ws = hw + 90, hw + 124
    rs = np.random.RandomState(hw)
    S = rs.standard_normal((Hs, Ws)).astype(F32)
    S[S == 0] = 1
    M = rs.randint(1, 256, size=(Hs, Ws)).astype(np.uint8)                  # never 0: a zero is the window's fill
    items = ec.crop_items(hw, (Hs, Ws), rs)
    B = len(items)
    assert ec.lane_trips(ec.crop_threads(hw), ec.CROP_CAP * ec.THREADS)[0] >= 2
    packed = np.array([[y0 * Ws + x0, Ws, (eh << 32) | ew, d4] for (y0, x0, eh, ew, d4) in items], np.int64)
    Sd, Md = dev(S), dev(M)
    x, y = _Out(B * hw * hw), _Out(B * hw * hw, torch.uint8)
    dclib.dc_crop_augment(Sd.data_ptr(), Md.data_ptr(), Hs * Ws, packed.ctypes.data, B, hw, x.ptr, y.ptr, None)
    xs, ys = x.host(B, hw, hw), y.host(B, hw, hw)
    for b, (y0, x0, eh, ew, d4) in enumerate(items):
        assert np.array_equal(xs[b].view(np.int32), ec.crop_ref(S, y0, x0, eh, ew, hw, d4).view(np.int32)), (b, items[b])
        assert np.array_equal(ys[b], ec.crop_ref(M, y0, x0, eh, ew, hw, d4)), (b, items[b])


# ---- 9. dc_round_window_u8: 256 workgroups per map --------------------------------------------------------------------------------------
def test_round_window_beyond_the_grid(dclib):
    r = ec.ROUND
    N, H, W, y0, y1, x0, x1 = (r[k] for k in ('N', 'H', 'W', 'y0', 'y1', 'x0', 'x1'))
    hh, ww = y1 - y0, x1 - x0
    p = np.random.RandomState(2).random_sample((N, H, W)).astype(F32)
    first = ec.ROUND_CAP * ec.THREADS
    half, above = F32(0.5), np.nextafter(F32(0.5), F32(1))
    for n in range(N):
        for i, v in ((first, half), (first + 1, above), (hh * ww - 1, half), (hh * ww - 2, above), (first - 1, above), (0, half)):
            p[n, y0 + i // ww, x0 + i % ww] = v
    pd = dev(p)
    out = _Out(N * hh * ww, torch.uint8)
    dclib.dc_round_window_u8(pd.data_ptr(), N, H, W, y0, y1, x0, x1, out.ptr, None)
    want = p[:, y0:y1, x0:x1].round().astype(np.uint8)
    assert want[0].ravel()[first] == 0 and want[1].ravel()[first + 1] == 1
    assert np.array_equal(out.host(N, hh, ww), want)
