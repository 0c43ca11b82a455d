"""Direct tests, through the C ABI on raw pointers, of the launch entry points that only whole-network tests used to reach:
the synchronised-BatchNorm pair (dc_bn_stats_reduce / dc_bn_stats_finalize_sums, dc_bn_bwd_apply_count), dc_bn_bwd_apply_finalize,
dc_bn_fold, the up-sampling branch (dc_upsample2x_drop_fwd / _bwd), the test-time-augmentation pair (dc_gather_maps, dc_tta_merge),
dc_scale_flat, and the stream / collective plumbing a step's tape replays (dc_event_record, dc_stream_wait_event, dc_comm_*).

Outputs are pre-filled with NaN (255 for uint8); references are float64 numpy.  Data movement and single exact fp32 operations
must be BIT-equal; where a tolerance is used its source is stated at the assertion: a rounding count, or the existing test of the
local entry point in tests/test_hip_ops.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import unet_numpy as on

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

U = 2.0 ** -24          # unit round-off of fp32
SLOTS = 8               # DC_ABOUND_SLOTS (include/dcunet.h)
_KEEP = []


@pytest.fixture(autouse=True)
def _keep_alive():
    """dev() temporaries must outlive the asynchronous launches that read them (raw pointers cross the C ABI)."""
    yield
    torch.cuda.synchronize()
    del _KEEP[:]


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _KEEP.append(t)
    return t


def nans(*shape, **kw):
    return torch.full(shape, float('nan'), device='cuda', **kw)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def dihedral_maps(H, W):
    """The 8 dihedral permutations of an H x W index image, flattened (rot90 of a non-square image changes its shape; the flat
    element count does not)."""
    idx = np.arange(H * W, dtype=np.int32).reshape(H, W)
    return np.stack([np.rot90(src, k).ravel() for src in (idx, np.fliplr(idx)) for k in range(4)]).astype(np.int32)


# ---- dc_gather_maps / dc_tta_merge / dc_scale_flat -----------------------------------------------------------------------------
def test_gather_maps_bit_exact(dclib):
    L = dclib
    H, W = 40, 56
    maps = dihedral_maps(H, W)
    assert len(set(m.tobytes() for m in maps)) == 8 and all(sorted(m) == list(range(H * W)) for m in maps)
    x = np.random.RandomState(1).standard_normal(H * W).astype(np.float32)
    for K in (8, 1):
        out = nans(K * H * W + 64)
        L.dc_gather_maps(dev(x).data_ptr(), dev(maps[:K]).data_ptr(), out.data_ptr(), K, H * W, None)
        o = host(out)
        assert bits_equal(o[:K * H * W].reshape(K, H * W), x[maps[:K]])
        assert np.isnan(o[K * H * W:]).all()
    # more elements than 4096 blocks x 256 threads: the grid-stride loop wraps
    n = 4096 * 256 + 12345
    big = np.random.RandomState(2).standard_normal(n).astype(np.float32)
    perm = np.random.RandomState(3).permutation(n).astype(np.int32)
    out = nans(n + 64)
    L.dc_gather_maps(dev(big).data_ptr(), dev(perm).data_ptr(), out.data_ptr(), 1, n, None)
    o = host(out)
    assert bits_equal(o[:n], big[perm]) and np.isnan(o[n:]).all()
    from deep_calcium_amd._lib import DcunetError
    with pytest.raises(DcunetError, match='dc_gather_maps'):
        L.dc_gather_maps(dev(x).data_ptr(), dev(maps).data_ptr(), out.data_ptr(), 0, H * W, None)


@pytest.mark.parametrize('K', [8, 1])
@pytest.mark.parametrize('threshold', [0.5, 0.3])
def test_tta_merge_mean_and_threshold(dclib, K, threshold):
    """mean_out == float32(sum_k float64(pred_k[inv_k]) / K), accumulated in table order in float64 -- bit for bit; mask is
    exactly m > threshold, with pixels placed on the threshold and one fp32 ulp either side."""
    L = dclib
    H, W, hs, ws = 40, 56, 33, 50
    rs = np.random.RandomState(K)
    maps = dihedral_maps(H, W)[:K]
    inv = np.stack([np.argsort(m, kind='stable') for m in maps]).astype(np.int32)
    # what the merge must see at pixel p from augmentation k, then carried into each prediction's own (augmented) frame
    target = rs.random_sample((K, H, W)).astype(np.float32)
    t32 = np.float32(threshold)
    on_thr = [t32, np.nextafter(t32, np.float32(0)), np.nextafter(t32, np.float32(1))]
    spots = [(0, 0), (32, 49), (10, 11), (32, 0), (0, 49), (17, 23)]
    for i, (y, x) in enumerate(spots[:3]):
        target[:, y, x] = on_thr[i]                          # all K equal: m is that fp32 value exactly
    for i, (y, x) in enumerate(spots[3:]):
        target[:, y, x] = on_thr[i]
        if K == 8:                                           # means next to the threshold from values that differ
            target[:4, y, x] += np.float32(0.125)
            target[4:, y, x] -= np.float32(0.125)
    preds = np.stack([target[k].ravel()[maps[k]] for k in range(K)])
    acc = np.zeros((H, W), np.float64)
    for k in range(K):
        acc += preds[k][inv[k]].reshape(H, W).astype(np.float64)
    m_ref = (acc / K)[:hs, :ws]
    assert np.array_equal(preds[0][inv[0]].reshape(H, W), target[0])
    for with_mean in (True, False):
        mask = torch.full((hs * ws + 64,), 255, dtype=torch.uint8, device='cuda')
        mean = nans(hs * ws + 64)
        L.dc_tta_merge(dev(preds).data_ptr(), dev(inv).data_ptr(), K, H, W, hs, ws, threshold, mask.data_ptr(),
                       mean.data_ptr() if with_mean else None, None)
        mk, mn = host(mask), host(mean)
        assert np.array_equal(mk[:hs * ws].reshape(hs, ws), (m_ref > threshold).astype(np.uint8))
        assert (mk[hs * ws:] == 255).all()
        if with_mean:
            assert bits_equal(mn[:hs * ws].reshape(hs, ws), m_ref.astype(np.float32)) and np.isnan(mn[hs * ws:]).all()
        else:
            assert np.isnan(mn).all()
    got = mk[:hs * ws].reshape(hs, ws)
    for i, (y, x) in enumerate(spots[:3]):
        v = float(on_thr[i])
        assert m_ref[y, x] == v and got[y, x] == (1 if v > threshold else 0), (y, x, v)
    from deep_calcium_amd._lib import DcunetError
    for bad in ((H + 1, ws), (hs, W + 1), (0, ws)):
        with pytest.raises(DcunetError, match='dc_tta_merge'):
            L.dc_tta_merge(dev(preds).data_ptr(), dev(inv).data_ptr(), K, H, W, bad[0], bad[1], threshold, mask.data_ptr(), None, None)


@pytest.mark.parametrize('n', [5, 1000003])
def test_scale_flat_is_one_fp32_multiply(dclib, n):
    """p[i] *= s: one exact-rounded fp32 product per element (1 000 003 > 2048 blocks x 256 threads: the loop wraps)."""
    L = dclib
    x = np.random.RandomState(n % 97).standard_normal(n + 64).astype(np.float32)
    s = np.float32(1.0 / 3.0)
    p = dev(x)
    L.dc_scale_flat(p.data_ptr(), n, float(s), None)
    o = host(p)
    assert bits_equal(o[:n], x[:n] * s) and bits_equal(o[n:], x[n:])
    from deep_calcium_amd._lib import DcunetError
    with pytest.raises(DcunetError, match='dc_scale_flat'):
        L.dc_scale_flat(p.data_ptr(), 0, 2.0, None)


# ---- UpSampling2D + Dropout ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,H,W,C,ldm', [(2, 5, 7, 8, 3), (1, 6, 10, 4, 1), (1, 3, 5, 512, 2), (3, 80, 72, 64, 1)])
def test_upsample_fwd_bwd_bit_exact(dclib, N, H, W, C, ldm):
    """keep = 1: pure data movement (np.repeat) forward, a 2x2 block sum in fp32 in the kernel's window order backward.
    Explicit masks at keep = 0.5: x * mask * 2, every factor exact.  Strided destination / source: the other columns of the
    buffer stay untouched."""
    L = dclib
    rs = np.random.RandomState(C + H)
    ld, off = ldm * C, (ldm - 1) * C
    x = rs.standard_normal((N, H, W, C)).astype(np.float32)
    dout = rs.standard_normal((N, 2 * H, 2 * W, ld)).astype(np.float32)
    mask = (rs.random_sample((N, 2 * H, 2 * W, C)) < 0.5).astype(np.uint8)
    up = x.repeat(2, axis=1).repeat(2, axis=2)
    for keep, m in ((1.0, None), (0.5, mask)):
        f = np.float32(1) if m is None else m.astype(np.float32) * np.float32(2)
        mptr = None if m is None else dev(m).data_ptr()
        out = nans(N, 2 * H, 2 * W, ld)
        L.dc_upsample2x_drop_fwd(dev(x).data_ptr(), out.data_ptr() + 4 * off, ld, mptr, keep, 0, None, 0, None, 0, N, H, W, C, None)
        o = host(out)
        assert bits_equal(o[..., off:], up * f)
        assert np.isnan(o[..., :off]).all()
        din = nans(N, H, W, C)
        L.dc_upsample2x_drop_bwd(dev(dout).data_ptr() + 4 * off, ld, mptr, keep, 0, din.data_ptr(), N, H, W, C, None)
        g = dout[..., off:] * f
        # window order 0..3 in fp32, from an accumulator that starts at +0 (four dropped negative gradients sum to +0, not -0)
        ref = (((np.float32(0) + g[:, 0::2, 0::2]) + g[:, 0::2, 1::2]) + g[:, 1::2, 0::2]) + g[:, 1::2, 1::2]
        assert ref.dtype == np.float32 and bits_equal(host(din), ref)


@pytest.mark.parametrize('keep', [1.0, 0.5, 0.75])
def test_upsample_abound_pair(dclib, keep):
    """abound_out = abound_in / keep: exact for keep 1 and 0.5; at 0.75 the kernel multiplies by fl(1 / keep), two roundings
    instead of one: within 2 x 2^-24 relative.  abound_in_ld == 0: one array; > 0: all DC_ABOUND_SLOTS replicas, each with its
    own stride, the gaps untouched.  One of the pair without the other is an argument error."""
    from deep_calcium_amd._lib import DcunetError
    L = dclib
    N, H, W, C = 1, 4, 6, 16
    rs = np.random.RandomState(5)
    x = dev(rs.standard_normal((N, H, W, C)).astype(np.float32))
    out = nans(N, 2 * H, 2 * W, C)
    mptr = None if keep >= 1 else dev((rs.random_sample((N, 2 * H, 2 * W, C)) < keep).astype(np.uint8)).data_ptr()

    def close(got, ab):
        want = (ab.astype(np.float64) / float(np.float32(keep)))
        if keep in (1.0, 0.5):
            return bits_equal(got, want.astype(np.float32))
        return bool((np.abs(got - want) <= 2 * U * np.abs(want)).all())

    ab = (rs.random_sample(C) * 30 + 0.1).astype(np.float32)
    abo = nans(C + 8)
    L.dc_upsample2x_drop_fwd(x.data_ptr(), out.data_ptr(), C, mptr, keep, 0, dev(ab).data_ptr(), 0, abo.data_ptr(), 0, N, H, W, C, None)
    o = host(abo)
    assert close(o[:C], ab) and np.isnan(o[C:]).all()
    ild, old = C + 4, C + 8
    abs_in = np.full((SLOTS, ild), np.nan, np.float32)
    abs_in[:, :C] = rs.random_sample((SLOTS, C)) * 30
    abo = nans(SLOTS, old)
    L.dc_upsample2x_drop_fwd(x.data_ptr(), out.data_ptr(), C, mptr, keep, 0, dev(abs_in).data_ptr(), ild, abo.data_ptr(), old, N, H, W, C, None)
    o = host(abo)
    assert close(o[:, :C], abs_in[:, :C]) and np.isnan(o[:, C:]).all()
    for pair in ((dev(ab).data_ptr(), None), (None, abo.data_ptr())):
        with pytest.raises(DcunetError, match='go together'):
            L.dc_upsample2x_drop_fwd(x.data_ptr(), out.data_ptr(), C, mptr, keep, 0, pair[0], 0, pair[1], 0, N, H, W, C, None)


# ---- dc_bn_fold ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [1, 24, 512])
def test_bn_fold(dclib, C):
    """scale = gamma / sqrt(mvar + eps), shift = beta + (bias - mmean) * scale.  Four fp32 roundings in the kernel (add, sqrt,
    divide; subtract / multiply-add for the shift): 4 x 2^-24 relative per output, the shift's scaled by |beta| + |bias - mmean| |scale|."""
    L = dclib
    rs = np.random.RandomState(C)
    f = np.float32
    gamma = (rs.uniform(0.5, 1.5, C) * rs.choice([-1.0, 1.0], C)).astype(f)
    beta, mmean, bias = (rs.standard_normal(C).astype(f) for _ in range(3))
    mvar = rs.uniform(0.01, 4.0, C).astype(f)
    eps = f(1e-3)
    g, b, mm, mv, bi = (a.astype(np.float64) for a in (gamma, beta, mmean, mvar, bias))
    sc_ref = g / np.sqrt(mv + float(eps))
    for with_bias in (True, False):
        bb = bi if with_bias else np.zeros(C)
        sh_ref = b + (bb - mm) * sc_ref
        sc, sh = nans(C + 4), nans(C + 4)
        L.dc_bn_fold(dev(gamma).data_ptr(), dev(beta).data_ptr(), dev(mmean).data_ptr(), dev(mvar).data_ptr(),
                     dev(bias).data_ptr() if with_bias else None, float(eps), sc.data_ptr(), sh.data_ptr(), C, None)
        s, h = host(sc), host(sh)
        assert np.isnan(s[C:]).all() and np.isnan(h[C:]).all()
        es = np.abs(s[:C] - sc_ref) / np.abs(sc_ref)
        eh = np.abs(h[:C] - sh_ref) / (np.abs(b) + np.abs(bb - mm) * np.abs(sc_ref))
        print('dc_bn_fold C=%d bias=%d: scale err %.2f u, shift err %.2f u' % (C, with_bias, es.max() / U, eh.max() / U))
        assert es.max() <= 4 * U and eh.max() <= 4 * U
    from deep_calcium_amd._lib import DcunetError
    with pytest.raises(DcunetError, match='dc_bn_fold'):
        L.dc_bn_fold(dev(gamma).data_ptr(), dev(beta).data_ptr(), dev(mmean).data_ptr(), None, None, 1e-3, sc.data_ptr(), sh.data_ptr(), C, None)


# ---- dc_bn_stats_reduce -> dc_bn_stats_finalize_sums -----------------------------------------------------------------------------
def _finalize_outputs(C):
    return dict(mean=nans(C), invstd=nans(C), scale=nans(C), shift=nans(C), abound=nans(C),
                mm=dev(np.full(C, 0.25, np.float32)), mv=dev(np.full(C, 2.0, np.float32)))


STATS_CASES = [(p, g, c, False) for p in (1, 257, 4097) for g in (1, 4) for c in (8, 512)] + [(1, 1, 8, True), (257, 4, 512, True)]


@pytest.mark.parametrize('parts,groups,C,constant', STATS_CASES)
def test_bn_stats_reduce_then_finalize_sums(dclib, parts, groups, C, constant):
    L = dclib
    rs = np.random.RandomState(parts + groups + C)
    nt = 16.0                                                # elements behind each partial row
    count = parts * groups * nt
    if constant:                                             # every element 3.25: the variance clamps at 0
        S = np.full((parts, groups, C), nt * 3.25)
        Q = np.full((parts, groups, C), nt * 3.25 * 3.25)
    else:
        mu, sig = rs.uniform(-2, 2, C), rs.uniform(0.5, 2.0, C)
        S = nt * mu + np.sqrt(nt) * sig * rs.standard_normal((parts, groups, C))
        Q = S * S / nt + sig * sig * (nt - 1) * rs.uniform(0.5, 1.5, (parts, groups, C))
    part = np.stack([S, Q], -1).reshape(parts, groups * C, 2)
    gamma = (rs.uniform(0.5, 1.5, C) * rs.choice([-1.0, 1.0], C)).astype(np.float32)
    beta = rs.uniform(-0.5, 0.5, C).astype(np.float32)
    pd, gd, bd = dev(part), dev(gamma), dev(beta)

    sums = nans(C, 2, dtype=torch.float64)
    L.dc_bn_stats_reduce(pd.data_ptr(), parts, groups, C, sums.data_ptr(), None)
    sm = host(sums)
    ref = np.stack([S.sum((0, 1)), Q.sum((0, 1))], -1)
    mag = np.stack([np.abs(S).sum((0, 1)), np.abs(Q).sum((0, 1))], -1)
    # two orders of at most parts * groups double additions: each within (n - 1) 2^-53 of sum |x|
    assert (np.abs(sm - ref) <= parts * groups * 2.0 ** -52 * mag).all()

    eps, mom = 1e-3, 0.9
    o = _finalize_outputs(C)
    L.dc_bn_stats_finalize_sums(sums.data_ptr(), C, count, eps, mom, o['mean'].data_ptr(), o['invstd'].data_ptr(), o['mm'].data_ptr(),
                                o['mv'].data_ptr(), gd.data_ptr(), bd.data_ptr(), o['scale'].data_ptr(), o['shift'].data_ptr(),
                                o['abound'].data_ptr(), None)
    a = _finalize_outputs(C)
    L.dc_bn_stats_finalize_affine(pd.data_ptr(), parts, groups, C, count, eps, mom, a['mean'].data_ptr(), a['invstd'].data_ptr(),
                                  a['mm'].data_ptr(), a['mv'].data_ptr(), gd.data_ptr(), bd.data_ptr(), a['scale'].data_ptr(),
                                  a['shift'].data_ptr(), a['abound'].data_ptr(), None)
    got = {k: host(v) for k, v in o.items()}
    mu_ref = ref[:, 0] / count
    var_ref = np.maximum(ref[:, 1] / count - mu_ref ** 2, 0.0)
    is_ref = 1.0 / np.sqrt(var_ref + float(np.float32(eps)))
    if constant:
        assert np.abs(var_ref).max() < 1e-9 and np.allclose(got['invstd'], 1 / np.sqrt(float(np.float32(eps))), rtol=2e-5)
    # the tolerances tests/test_hip_ops.py::test_batchnorm_relu_dropout_fwd_bwd holds the local finalize to
    assert np.allclose(got['mean'], mu_ref, atol=2e-6)
    assert np.allclose(got['invstd'], is_ref, rtol=2e-5)
    assert np.allclose(got['mm'], 0.25 * mom + mu_ref * (1 - mom), atol=1e-6)
    assert np.allclose(got['mv'], 2.0 * mom + var_ref * (1 - mom), rtol=1e-5)
    # ... and test_bn_relu_on_load_conv_convT_wgrad_head for the bound; scale / shift carry invstd's and mean's tolerances through
    # gamma * invstd and beta - mean * scale
    assert np.allclose(got['abound'], np.abs(gamma) * np.sqrt(count) + np.abs(beta), rtol=1e-6)
    sc_ref = gamma.astype(np.float64) * is_ref
    assert np.allclose(got['scale'], sc_ref, rtol=2e-5, atol=0)
    assert (np.abs(got['shift'] - (beta - mu_ref * sc_ref)) <= 2e-5 * (np.abs(beta) + np.abs(mu_ref * sc_ref)) + 2e-6 * np.abs(sc_ref)).all()
    # include/dcunet.h: "With one rank (or count == pixels) the results equal the local entry points'" -- bit for bit
    for k in o:
        assert bits_equal(got[k], host(a[k])), k
    # scale / shift / abound are optional
    m2, i2 = nans(C), nans(C)
    L.dc_bn_stats_finalize_sums(sums.data_ptr(), C, count, eps, -1.0, m2.data_ptr(), i2.data_ptr(), None, None, None, None, None, None, None, None)
    assert bits_equal(host(m2), got['mean']) and bits_equal(host(i2), got['invstd'])
    from deep_calcium_amd._lib import DcunetError
    with pytest.raises(DcunetError, match='scale needs'):
        L.dc_bn_stats_finalize_sums(sums.data_ptr(), C, count, eps, -1.0, m2.data_ptr(), i2.data_ptr(), None, None, None, None,
                                    o['scale'].data_ptr(), o['shift'].data_ptr(), None, None)


# ---- dc_bn_bwd_apply_count -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,drop', [(8, 'mask'), (64, 'rng'), (32, 'none'), (256, 'rng'), (4, 'mask')])
def test_bn_bwd_apply_count_two_shards_meet_the_whole_batch(dclib, C, drop):
    """Synchronised BatchNorm backward: each shard runs with count = the WHOLE batch's elements per channel and the global
    dgamma / dbeta; the concatenated dz must meet the float64 bn_train_bwd of the whole batch at the 3e-5 of
    test_batchnorm_relu_dropout_fwd_bwd.  Dropout: explicit masks, or the counter hash under the shard's seed."""
    from deep_calcium_amd import parallel
    from deep_calcium_amd._lib import DcunetError
    L = dclib
    N, H, W = 4, 6, 10
    M, per = N * H * W, (N // 2) * H * W
    rs = np.random.RandomState(C)
    keep = 1.0 if drop == 'none' else 0.75
    seed = 0xA5A5A5A5DEADBEEF
    z = (rs.standard_normal((N, H, W, C)) * 1.7 + 0.4).astype(np.float32)
    gamma = rs.uniform(0.5, 1.5, C).astype(np.float32)
    beta = rs.uniform(-0.5, 0.5, C).astype(np.float32)
    ld = 2 * C
    dabuf = rs.standard_normal((N, H, W, ld)).astype(np.float32)
    da = dabuf[..., C:]
    if drop == 'mask':
        mask = (rs.random_sample((N, H, W, C)) < keep).astype(np.uint8)
    elif drop == 'rng':
        mask = on.hash_keep_mask(seed, M * C, keep).reshape(N, H, W, C)
    else:
        mask = np.ones((N, H, W, C), np.uint8)
    fac = mask / keep if keep < 1 else 1.0
    y_ref, cache = on.bn_train_fwd(z.astype(np.float64), gamma.astype(np.float64), beta.astype(np.float64))
    dy = da.astype(np.float64) * fac * (y_ref > 0)
    dz_ref, dg_ref, db_ref = on.bn_train_bwd(dy, gamma.astype(np.float64), cache)
    mean, invstd = dev(cache[2].astype(np.float32)), dev(cache[1].astype(np.float32))
    gd, bd = dev(gamma), dev(beta)
    dgd, dbd = dev(dg_ref.astype(np.float32)), dev(db_ref.astype(np.float32))

    def shard(r, count, which='count'):
        sl = slice(r * (N // 2), (r + 1) * (N // 2))
        blocks = L.dc_bn_bwd_blocks(per, C)
        dz, dbp, amax = nans(N // 2, H, W, C), nans(blocks, C), nans(blocks)
        if drop == 'mask':
            mptr, sd = dev(mask[sl]).data_ptr(), 0
        else:
            mptr, sd = None, (parallel.shard_drop_seed(seed, per * C, r) if drop == 'rng' else 0)
        head = (dev(dabuf[sl]).data_ptr() + 4 * C, ld, dev(z[sl]).data_ptr(), mean.data_ptr(), invstd.data_ptr(), gd.data_ptr(),
                bd.data_ptr(), mptr, keep, sd, dgd.data_ptr(), dbd.data_ptr(), dz.data_ptr(), dbp.data_ptr(), amax.data_ptr(), per)
        if which == 'count':
            L.dc_bn_bwd_apply_count(*head, float(count), C, None)
        else:
            L.dc_bn_bwd_apply(*head, C, None)
        return [host(t) for t in (dz, dbp, amax)]

    parts = [shard(r, M) for r in range(2)]
    dz = np.concatenate([p[0] for p in parts])
    err = np.abs(dz - dz_ref).max()
    print('dc_bn_bwd_apply_count C=%d %s: max|dz - ref| = %.3e (scale %.3e)' % (C, drop, err, np.abs(dz_ref).max()))
    assert err < 3e-5 * max(np.abs(dz_ref).max(), 1)
    for p in parts:
        assert p[2].max() == np.abs(p[0]).max()              # per-block max |dz|
        cols = p[0].reshape(-1, C).astype(np.float64)        # dbias_partial: an fp32 sum of `per` values, any order: (n - 1) u sum |x|
        assert (np.abs(p[1].astype(np.float64).sum(0) - cols.sum(0)) <= per * U * np.abs(cols).sum(0)).all()
    # a shard that forgot the global count (M/2 instead of M) misses the whole-batch dz
    wrong = np.concatenate([shard(r, per)[0] for r in range(2)])
    assert np.abs(wrong - dz_ref).max() > 1e-3
    # count == pixels: the local entry point, bit for bit
    for a, b in zip(shard(1, per), shard(1, per, 'local')):
        assert bits_equal(a, b)
    with pytest.raises(DcunetError, match='count < pixels'):
        shard(0, per - 1)


# ---- dc_bn_bwd_apply_finalize ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C', [8, 48])
@pytest.mark.parametrize('case', ['random', 'zero', 'last_block', 'one_block'])
def test_bn_bwd_apply_finalize(dclib, C, case):
    """dbias = fixed-order column sum of dbias_partial[blocks][C] against float64 (2e-5 of scale, as every gradient sum in
    test_batchnorm_relu_dropout_fwd_bwd); scale[0] bit-equal to dc_pow2_scale_from_absmax on the same maxima."""
    from deep_calcium_amd._lib import DcunetError
    L = dclib
    blocks = 1 if case == 'one_block' else 300
    rs = np.random.RandomState(C + blocks)
    dbp = rs.standard_normal((blocks, C)).astype(np.float32)
    amax = np.abs(rs.standard_normal(blocks)).astype(np.float32) * 1e-3
    if case == 'zero':
        amax[:] = 0
    elif case == 'last_block':
        amax[-1] = 7.25
    target = 1024.0
    db, sc, sc2 = nans(C + 4), nans(4), nans(4)
    L.dc_bn_bwd_apply_finalize(dev(dbp).data_ptr(), dev(amax).data_ptr(), blocks, C, target, db.data_ptr(), sc.data_ptr(), None)
    L.dc_pow2_scale_from_absmax(dev(amax).data_ptr(), blocks, target, sc2.data_ptr(), None)
    d, s, s2 = host(db), host(sc), host(sc2)
    ref = dbp.astype(np.float64).sum(0)
    assert np.abs(d[:C] - ref).max() < 2e-5 * max(np.abs(ref).max(), 1) and np.isnan(d[C:]).all()
    assert bits_equal(s, s2) and np.isnan(s[1:]).all()
    mx = float(amax.max())
    assert s[0] == (1.0 if mx == 0 else 2.0 ** np.floor(np.log2(target / mx)))
    if case == 'last_block':
        assert s[0] == 128.0
    # (NULL, NULL): only dbias is written
    db2 = nans(C + 4)
    L.dc_bn_bwd_apply_finalize(dev(dbp).data_ptr(), None, blocks, C, target, db2.data_ptr(), None, None)
    assert bits_equal(host(db2), d)
    for pair in ((dev(amax).data_ptr(), None), (None, sc.data_ptr())):
        with pytest.raises(DcunetError, match='go together'):
            L.dc_bn_bwd_apply_finalize(dev(dbp).data_ptr(), pair[0], blocks, C, target, db.data_ptr(), pair[1], None)


# ---- what a step's tape replays besides kernels: stream ordering and the collectives ---------------------------------------------
def test_event_record_and_stream_wait_order_two_streams(dclib):
    """dc_event_record on one stream + dc_stream_wait_event on another: the second stream's launch sees everything the first
    queued before the record (20 fills of a 256 MiB buffer, then x2 on the other stream)."""
    L = dclib
    n = 1 << 26
    buf = torch.zeros(n, device='cuda')
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    ev, t0, t1 = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    L.dc_event_create_sync(ctypes.byref(ev))
    L.dc_event_create(ctypes.byref(t0))
    L.dc_event_create(ctypes.byref(t1))
    try:
        L.dc_event_record(t0, s1.cuda_stream)
        for v in range(1, 21):
            L.dc_fill(buf.data_ptr(), n, float(v), s1.cuda_stream)
        L.dc_event_record(ev, s1.cuda_stream)
        L.dc_event_record(t1, s1.cuda_stream)
        L.dc_stream_wait_event(s2.cuda_stream, ev)
        L.dc_scale_flat(buf.data_ptr(), n, 2.0, s2.cuda_stream)
        torch.cuda.synchronize()
        assert float(buf.min()) == 40.0 and float(buf.max()) == 40.0
        ms = ctypes.c_float(-1.0)
        L.dc_event_elapsed_ms(t0, t1, ctypes.byref(ms))
        assert 0.0 < ms.value < 1000.0
    finally:
        for e in (ev, t0, t1):
            L.dc_event_destroy(e)


_ONE_RANK_COLLECTIVES = r'''
import ctypes, sys
import numpy as np
import torch
from deep_calcium_amd import _lib
L = _lib.lib()
ident = ctypes.create_string_buffer(128)                    # DC_COMM_ID_BYTES
L.dc_comm_unique_id(ident)
comm = ctypes.c_void_p()
L.dc_comm_init_rank(ctypes.byref(comm), ident, 1, 0)
st = torch.cuda.Stream()
rs = np.random.RandomState(0)
a, b = rs.standard_normal(100003).astype(np.float32), rs.standard_normal(12)
x, y = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
torch.cuda.synchronize()
L.dc_comm_all_reduce_sum(comm, x.data_ptr(), x.numel(), st.cuda_stream)
L.dc_comm_all_reduce_sum_f64(comm, y.data_ptr(), y.numel(), st.cuda_stream)
L.dc_comm_group_start()
L.dc_comm_all_reduce_sum(comm, x.data_ptr(), 4096, st.cuda_stream)
L.dc_comm_all_reduce_sum_f64(comm, y.data_ptr(), 5, st.cuda_stream)
L.dc_comm_group_end()
torch.cuda.synchronize()
ok = x.cpu().numpy().tobytes() == a.tobytes() and y.cpu().numpy().tobytes() == b.tobytes()
L.dc_comm_destroy(comm)
print('ONE_RANK_OK' if ok else 'ONE_RANK_MISMATCH')
'''


def test_one_rank_all_reduce_is_the_identity():
    """dc_comm_all_reduce_sum / _f64, alone and between dc_comm_group_start / _end, on a one-rank communicator: the sum over one
    rank leaves every bit in place (fp32 and fp64).  Run in a child process, as tests/test_comm_gpu.py runs RCCL."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root, HSA_ENABLE_IPC_MODE_LEGACY='0')
    r = subprocess.run([sys.executable, '-c', _ONE_RANK_COLLECTIVES], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'ONE_RANK_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
