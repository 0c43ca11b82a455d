"""UNet1D training on the device (include/dcunet.h, UNet1D training section; deep_calcium_amd/unet1d_train.py, spikes_fit.py)
against the float64 oracle of tests/_unet1d_train_ref.py (torch CPU autograd, plus a hand-written numpy backward of the head).

Tolerances are the project's: forward tensors, probabilities and every gradient tensor within 1e-4 * max |reference| of that
tensor; what only moves values (pooling routing, up-sampling, dropout masks) exact; repeated calls bit-identical.  Every test
prints the figure it asserts on."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _unet1d_ref as ref              # noqa: E402
import _unet1d_train_ref as tref       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -12345.5


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()


def _empty(n, fill=POISON, dtype=torch.float32):
    return torch.full((int(n),), fill, dtype=dtype, device='cuda')


def _rel(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-300))


# ---- BatchNorm statistics --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(1, 1, 4), (3, 37, 12), (2, 300, 32)], ids=lambda s: 'x'.join(map(str, s)))
def test_conv1d_stats(dclib, shape):
    N, T, C = shape
    z = (np.random.RandomState(T).randn(N, T, C) * 2. + 3.).astype(np.float32)
    zd = _dev(z)
    blocks = dclib.dc_conv1d_stats_blocks(N * T, C)
    assert blocks >= 1
    outs = []
    for fill in (0., 7.):
        part = torch.full((blocks, C, 2), fill, dtype=torch.float64, device='cuda')
        dclib.dc_conv1d_stats(zd.data_ptr(), C, part.data_ptr(), N * T, C, _st())
        torch.cuda.synchronize()
        outs.append(part.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])                       # every row written, the same bits twice
    got = outs[0].sum(0)
    z64 = z.astype(np.float64).reshape(-1, C)
    want = np.stack([z64.sum(0), (z64 * z64).sum(0)], 1)
    err = _rel(got, want)
    print('dc_conv1d_stats %r (%d blocks): %.3g' % (shape, blocks, err))
    assert err <= 1e-4
    # and through the finalize launch the training engine uses: mean / invstd of the batch
    mean, invstd = _empty(C), _empty(C)
    part = _dev(outs[0])
    dclib.dc_bn_stats_finalize(part.data_ptr(), blocks, 1, C, float(N * T), 1e-3, -1.0, mean.data_ptr(), invstd.data_ptr(), None, None, _st())
    torch.cuda.synchronize()
    assert _rel(mean.cpu().numpy(), z64.mean(0)) <= 1e-4
    assert _rel(invstd.cpu().numpy(), 1. / np.sqrt(z64.var(0) + 1e-3)) <= 1e-4


def test_conv1d_stats_reads_its_channel_slice(dclib):
    N, T, C, ld = 2, 19, 8, 24
    buf = np.random.RandomState(1).randn(N, T, ld).astype(np.float32)
    bd = _dev(buf)
    blocks = dclib.dc_conv1d_stats_blocks(N * T, C)
    part = torch.zeros((blocks, C, 2), dtype=torch.float64, device='cuda')
    dclib.dc_conv1d_stats(bd.data_ptr() + 4 * 16, ld, part.data_ptr(), N * T, C, _st())
    torch.cuda.synchronize()
    z64 = buf[..., 16:].astype(np.float64).reshape(-1, C)
    assert _rel(part.cpu().numpy().sum(0), np.stack([z64.sum(0), (z64 * z64).sum(0)], 1)) <= 1e-4


# ---- conv gradients --------------------------------------------------------------------------------------------------
GRAD_SHAPES = [(1, 16, 4, 4), (3, 37, 12, 4), (2, 70, 32, 96), (2, 1, 4, 8), (2, 2, 8, 4)]


@functools.lru_cache(maxsize=None)
def _conv_case(shape):
    N, T, Cin, Cout = shape
    rs = np.random.RandomState(N * 1000 + T + Cin + Cout)
    x = rs.randn(N, T, Cin).astype(np.float32)
    k = (rs.randn(5, Cin, Cout) * np.sqrt(2. / (5 * Cin))).astype(np.float32)
    dz = rs.randn(N, T, Cout).astype(np.float32)
    dx, dw = tref.conv_grads(x, k, dz)
    for a in (x, k, dz, dx, dw):
        a.setflags(write=False)
    return x, k, dz, dx, dw


@pytest.mark.parametrize('shape', GRAD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_data_gradient_is_the_forward_on_repacked_weights(dclib, shape):
    N, T, Cin, Cout = shape
    x, k, dz, dx_want, _ = _conv_case(shape)
    kd, wp = _dev(k), _empty(k.size)
    dclib.dc_pack_weights(kd.data_ptr(), wp.data_ptr(), 5, Cout, Cin, Cin * Cout, 1, Cout, 1, _st())     # flipped, Cin <-> Cout
    ones, zeros = torch.ones(Cin, device='cuda'), torch.zeros(Cin, device='cuda')
    dzd, dx = _dev(dz), _empty(N * T * Cin)
    dclib.dc_conv1d_k5_fwd(dzd.data_ptr(), wp.data_ptr(), ones.data_ptr(), zeros.data_ptr(), 0, dx.data_ptr(), Cin, N, T, Cout, Cin, _st())
    torch.cuda.synchronize()
    err = _rel(dx.cpu().numpy().reshape(N, T, Cin), dx_want)
    print('data gradient %r: %.3g' % (shape, err))
    assert err <= 1e-4


def _run_wgrad(dclib, x, dz, fill):
    N, T, Cin = x.shape
    Cout = dz.shape[2]
    n_ws = dclib.dc_conv1d_k5_wgrad_ws_floats(N, T, Cin, Cout)
    assert n_ws >= 5 * Cin * Cout * dclib.dc_conv1d_k5_wgrad_blocks(N, T, Cin, Cout)
    xd, dzd, dw, ws = _dev(x), _dev(dz), _empty(5 * Cin * Cout), _empty(n_ws, fill)
    dclib.dc_conv1d_k5_wgrad(xd.data_ptr(), dzd.data_ptr(), dw.data_ptr(), ws.data_ptr(), N, T, Cin, Cout, _st())
    torch.cuda.synchronize()
    return dw.cpu().numpy().reshape(5, Cin, Cout)


# (3,5,4,4): three traces shorter than the halo -- a read across a trace boundary shows; (6,200,4,4): more than one contraction
# partition; (2,70,96,32): more than one input-channel chunk; (2,70,36,68): both channel counts past 32 (the 2 x 2 wave arrangement),
# ragged on both channel blocks, two tiles per trace
@pytest.mark.parametrize('shape', GRAD_SHAPES + [(3, 5, 4, 4), (6, 200, 4, 4), (2, 70, 96, 32), (2, 70, 36, 68)], ids=lambda s: 'x'.join(map(str, s)))
def test_conv1d_k5_wgrad(dclib, shape):
    N, T, Cin, Cout = shape
    x, k, dz, _, dw_want = _conv_case(shape)
    got = _run_wgrad(dclib, x, dz, 0.)
    err = _rel(got, dw_want)
    print('dc_conv1d_k5_wgrad %r (%d partitions): %.3g' % (shape, dclib.dc_conv1d_k5_wgrad_blocks(N, T, Cin, Cout), err))
    assert err <= 1e-4
    assert np.array_equal(got, _run_wgrad(dclib, x, dz, 1e30))       # a dirty workspace changes no bit; twice the same bits
    if shape == (6, 200, 4, 4):
        assert dclib.dc_conv1d_k5_wgrad_blocks(N, T, Cin, Cout) > 1


def test_conv1d_k5_wgrad_never_crosses_traces(dclib):
    """A huge trace beside a zero-gradient... the other way round: trace 1's x is huge but its dz is zero, so it must add nothing."""
    x, k, dz, _, _ = _conv_case((3, 5, 4, 4))
    x2, dz2 = x.copy(), dz.copy()
    x2[1] = 1e6
    dz2[1] = 0.
    _, want = tref.conv_grads(x2[[0, 2]], k, dz2[[0, 2]])
    got = _run_wgrad(dclib, x2, dz2, 0.)
    assert _rel(got, want) <= 1e-4


@pytest.mark.parametrize('shape', [(1, 16, 4), (3, 37, 32), (2, 2100, 8)], ids=lambda s: 'x'.join(map(str, s)))
def test_conv1d_k5_c1_wgrad(dclib, shape):
    N, T, Cout = shape
    rs = np.random.RandomState(T)
    x = rs.randn(N, T, 1).astype(np.float32)
    k = rs.randn(5, 1, Cout).astype(np.float32)
    dz = rs.randn(N, T, Cout).astype(np.float32)
    _, want = tref.conv_grads(x, k, dz)
    outs = []
    for fill in (0., 1e30):
        xd, dzd, dw = _dev(x), _dev(dz), _empty(5 * Cout)
        ws = _empty(dclib.dc_conv1d_k5_c1_wgrad_ws_floats(N, T, Cout), fill)
        dclib.dc_conv1d_k5_c1_wgrad(xd.data_ptr(), dzd.data_ptr(), dw.data_ptr(), ws.data_ptr(), N, T, Cout, _st())
        torch.cuda.synchronize()
        outs.append(dw.cpu().numpy().reshape(5, 1, Cout))
    err = _rel(outs[0], want)
    print('dc_conv1d_k5_c1_wgrad %r: %.3g' % (shape, err))
    assert err <= 1e-4 and np.array_equal(outs[0], outs[1])


# ---- pooling backward ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 2, 7, 64])
def test_maxpool1d_2_bwd_routes_exactly(dclib, T):
    N, C = 3, 8
    rs = np.random.RandomState(T)
    cat = np.maximum(rs.randn(N, T, 3 * C), 0.).astype(np.float32)          # post-ReLU: exact zero ties in about a quarter of the pairs
    cat[:, :, 2 * C] = 1.5                                                  # and a channel of equal positives
    x = cat[..., 2 * C:]
    dy = rs.randn(N, T // 2, C).astype(np.float32)
    dcat = rs.randn(N, T, 3 * C).astype(np.float32)
    want = tref.pool2_bwd(x, dy).astype(np.float32) + dcat[..., 2 * C:]     # one fp32 addition per element: exact to compare
    catd, dyd, dcatd = _dev(cat), _dev(dy if T > 1 else np.zeros((N, 1, C), np.float32)), _dev(dcat)
    ld = C + 8
    dx = torch.full((N, T, ld), POISON, dtype=torch.float32, device='cuda')
    dclib.dc_maxpool1d_2_bwd(dyd.data_ptr(), catd.data_ptr() + 4 * 2 * C, 3 * C, dcatd.data_ptr() + 4 * 2 * C, 3 * C,
                             dx.data_ptr() + 4 * 4, ld, N, T, C, _st())
    torch.cuda.synchronize()
    got = dx.cpu().numpy()
    assert (got[..., :4] == POISON).all() and (got[..., 4 + C:] == POISON).all()        # channels outside the slice untouched
    assert np.array_equal(got[..., 4:4 + C], want)
    if T >= 2:
        ties = (x[:, 0:T // 2 * 2:2] == x[:, 1:T // 2 * 2:2])
        assert ties.any()
    # without a skip gradient: the routing alone
    dx2 = _empty(N * T * C)
    dclib.dc_maxpool1d_2_bwd(dyd.data_ptr(), catd.data_ptr() + 4 * 2 * C, 3 * C, None, 0, dx2.data_ptr(), C, N, T, C, _st())
    torch.cuda.synchronize()
    assert np.array_equal(dx2.cpu().numpy().reshape(N, T, C), tref.pool2_bwd(x, dy).astype(np.float32))


# ---- up-sampling + dropout -------------------------------------------------------------------------------------------
def _up_fwd(dclib, x, ld, mask, keep, seed):
    N, T, C = x.shape
    xd = _dev(x)
    out = torch.full((N, 2 * T, ld), POISON, dtype=torch.float32, device='cuda')
    md = _dev(mask) if mask is not None else None
    dclib.dc_upsample1d_2x_drop_fwd(xd.data_ptr(), out.data_ptr(), ld, md.data_ptr() if md is not None else None, keep, seed, N, T, C, _st())
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _up_bwd(dclib, dout, C, mask, keep, seed):
    N, T2, ld = dout.shape
    dd, din = _dev(dout), _empty(N * (T2 // 2) * C)
    md = _dev(mask) if mask is not None else None
    dclib.dc_upsample1d_2x_drop_bwd(dd.data_ptr(), ld, md.data_ptr() if md is not None else None, keep, seed, din.data_ptr(), N, T2 // 2, C, _st())
    torch.cuda.synchronize()
    return din.cpu().numpy().reshape(N, T2 // 2, C)


@pytest.mark.parametrize('T', [1, 5, 64])
def test_upsample1d_2x_drop(dclib, T):
    N, C, ld, keep = 2, 8, 12, 0.75
    rs = np.random.RandomState(T)
    x = rs.randn(N, T, C).astype(np.float32)
    mask = (rs.uniform(size=(N, 2 * T, C)) < keep).astype(np.uint8)
    dout = rs.randn(N, 2 * T, ld).astype(np.float32)
    # explicit mask against the oracle
    got = _up_fwd(dclib, x, ld, mask, keep, 0)
    want = np.repeat(x.astype(np.float64), 2, axis=1) * mask / keep
    assert (got[..., C:] == POISON).all() and _rel(got[..., :C], want) <= 1e-6
    assert np.array_equal(got[..., :C] == 0, (mask == 0) | (np.repeat(x, 2, axis=1) == 0))
    gin = _up_bwd(dclib, dout, C, mask, keep, 0)
    gw = (dout[..., :C].astype(np.float64) * mask / keep).reshape(N, T, 2, C).sum(2)
    assert _rel(gin, gw) <= 1e-6
    # keep = 1: dc_upsample1d_2x_fwd bit for bit
    plain = torch.full((N, 2 * T, ld), POISON, dtype=torch.float32, device='cuda')
    xd = _dev(x)
    dclib.dc_upsample1d_2x_fwd(xd.data_ptr(), plain.data_ptr(), ld, N, T, C, _st())
    torch.cuda.synchronize()
    assert np.array_equal(_up_fwd(dclib, x, ld, None, 1.0, 5), plain.cpu().numpy())
    # the counter RNG: forward and backward see the same mask, about `keep` of it set, another seed another mask
    ones = np.ones((N, T, C), np.float32)
    m_f = _up_fwd(dclib, ones, C, None, keep, 1234)
    assert set(np.unique(m_f)) <= {0., np.float32(1. / keep)}
    m_b = _up_bwd(dclib, np.ones((N, 2 * T, C), np.float32), C, None, keep, 1234)
    assert np.array_equal(m_b, m_f.reshape(N, T, 2, C).sum(2))
    if T == 64:
        assert abs((m_f > 0).mean() - keep) < 0.05
        assert not np.array_equal(m_f, _up_fwd(dclib, ones, C, None, keep, 1235))


# ---- the head --------------------------------------------------------------------------------------------------------
def _head_fwd(dclib, a, kh, bh, pool, y, wpos=2., wneg=1.):
    N, T, C = a.shape
    ad, kd, bd, yd = _dev(a), _dev(kh), _dev(bh), _dev(y)
    blocks = dclib.dc_spike_head_train_fwd_blocks(N, T)
    p, part, sums = _empty(N * T), _empty(blocks * 8), torch.zeros(8, dtype=torch.float64, device='cuda')
    dclib.dc_spike_head_train_fwd(ad.data_ptr(), kd.data_ptr(), bd.data_ptr(), pool, yd.data_ptr(), wpos, wneg, p.data_ptr(),
                                  part.data_ptr(), N, T, C, _st())
    dclib.dc_reduce_partials_f64(part.data_ptr(), blocks, 8, sums.data_ptr(), _st())
    torch.cuda.synchronize()
    return p.cpu().numpy().reshape(N, T), sums.cpu().numpy()


def _head_bwd(dclib, a, kh, bh, pool, y, wpos=2., wneg=1.):
    N, T, C = a.shape
    ad, kd, bd, yd = _dev(a), _dev(kh), _dev(bh), _dev(y)
    blocks = dclib.dc_spike_head_train_bwd_blocks(N, T)
    L = 2 * C + 2
    da, part, g, tmp = _empty(N * T * C), _empty(blocks * L), _empty(L), _empty(32 * L)
    dclib.dc_spike_head_train_bwd(ad.data_ptr(), kd.data_ptr(), bd.data_ptr(), pool, yd.data_ptr(), wpos, wneg, da.data_ptr(),
                                  part.data_ptr(), N, T, C, _st())
    dclib.dc_reduce_partials(part.data_ptr(), blocks, L, 1.0, g.data_ptr(), tmp.data_ptr(), _st())
    torch.cuda.synchronize()
    g = g.cpu().numpy()
    return da.cpu().numpy().reshape(N, T, C), g[:2 * C].reshape(C, 2), g[2 * C:]


@functools.lru_cache(maxsize=None)
def _head_case(pool, C, T):
    """Random head inputs whose float64 probabilities stay 1e-4 away from the rounding threshold 0.5 (the metric sums are then
    the same integers in fp32): the first seed for which the ORACLE says so."""
    for seed in range(50):
        rs = np.random.RandomState(pool * 1000 + T * 10 + C + 7919 * seed)
        a = np.maximum(rs.randn(3, T, C), 0.).astype(np.float32)
        kh = (rs.randn(C, 2) * np.sqrt(2. / C)).astype(np.float32)
        bh = (rs.randn(2) * 0.1).astype(np.float32)
        y = (rs.uniform(size=(3, T)) < 0.3).astype(np.uint8)
        if (np.abs(ref.head(a.astype(np.float64), kh, bh, pool) - 0.5) > 1e-4).all():
            return a, kh, bh, y
    raise AssertionError('no seed keeps the oracle away from p = 0.5')


@pytest.mark.parametrize('C', [4, 32])
@pytest.mark.parametrize('pool', [1, 2, 5, 64])
def test_spike_head_train(dclib, pool, C):
    for T in (1, 3, 40, 300):                   # 300: past both kernels' tiles (192 / 128), the window reaches across them
        a, kh, bh, y = _head_case(pool, C, T)
        loss_w, p_w, da_w, dkh_w, dbh_w = tref.head_loss_grads(a, kh, bh, pool, y)
        da_n, dkh_n, dbh_n = tref.head_bwd_np(a, kh, bh, pool, y)                 # the second opinion agrees with autograd
        assert _rel(da_n, da_w) < 1e-9 and _rel(dkh_n, dkh_w) < 1e-9 and _rel(dbh_n, dbh_w) < 1e-9
        p, sums = _head_fwd(dclib, a, kh, bh, pool, y)
        # the same probabilities as the inference head, bit for bit
        ad, kd, bd, p_inf = _dev(a), _dev(kh), _dev(bh), _empty(3 * T)
        dclib.dc_spike_head_fwd(ad.data_ptr(), kd.data_ptr(), bd.data_ptr(), pool, p_inf.data_ptr(), 3, T, C, _st())
        torch.cuda.synchronize()
        assert np.array_equal(p, p_inf.cpu().numpy().reshape(3, T))
        e_p, e_l = float(np.abs(p - p_w).max()), abs(sums[0] / (3 * T) - loss_w) / abs(loss_w)
        assert (np.abs(p_w - 0.5) > 1e-4).all()                                     # no sample at the rounding threshold
        assert np.array_equal(sums[1:5], tref.metric_sums(p_w, y)) and (sums[5:] == 0).all()
        da, dkh, dbh = _head_bwd(dclib, a, kh, bh, pool, y)
        errs = (_rel(da, da_w), _rel(dkh, dkh_w), _rel(dbh, dbh_w))
        print('head pool=%d C=%d T=%d: |dp| %.3g loss %.3g  da %.3g dkh %.3g dbh %.3g' % ((pool, C, T, e_p, e_l) + errs))
        assert e_p <= 1e-4 and e_l <= 1e-4 and max(errs) <= 1e-4
        da2, dkh2, dbh2 = _head_bwd(dclib, a, kh, bh, pool, y)
        assert np.array_equal(da, da2) and np.array_equal(dkh, dkh2) and np.array_equal(dbh, dbh2)


def test_spike_head_train_saturated_logits_stay_finite(dclib):
    """p exactly 0 and exactly 1 in fp32: the loss and every gradient stay finite, and agree with float64."""
    C, T, pool = 4, 6, 3
    a = np.zeros((1, T, C), np.float32)
    a[0, :, 0] = [200., 200., 200., -200., -200., -200.]
    kh = np.zeros((C, 2), np.float32)
    kh[0, 1] = 1.
    bh = np.zeros(2, np.float32)
    y = np.array([[1, 0, 1, 0, 1, 0]], np.uint8)
    p, sums = _head_fwd(dclib, a, kh, bh, pool, y)
    assert (p[0, :3] == 1.).all() and (p[0, 4:] == 0.).all()
    loss_w, p_w, da_w, dkh_w, dbh_w = tref.head_loss_grads(a, kh, bh, pool, y)
    assert np.isfinite(sums).all() and abs(sums[0] / T - loss_w) <= 1e-4 * loss_w
    da, dkh, dbh = _head_bwd(dclib, a, kh, bh, pool, y)
    assert np.isfinite(da).all() and np.isfinite(dkh).all() and np.isfinite(dbh).all()
    scale = max(np.abs(dkh_w).max(), 1e-3)               # the float64 gradients are ~1e-80 here: compare on the loss' own scale
    assert np.abs(dkh - dkh_w).max() <= 1e-4 * scale and np.abs(da - da_w).max() <= 1e-4 * scale


def test_spike_head_metric_rounding_is_half_to_even(dclib):
    """p == 0.5 exactly (equal logits) rounds to 0: no predicted spike, every true spike a false negative."""
    C, T = 4, 5
    a, kh, bh = np.zeros((1, T, C), np.float32), np.zeros((C, 2), np.float32), np.zeros(2, np.float32)
    y = np.array([[1, 0, 1, 0, 0]], np.uint8)
    p, sums = _head_fwd(dclib, a, kh, bh, 1, y)
    assert (p == 0.5).all() and np.array_equal(sums[1:5], [0., 0., 2., 2.])


# ---- the whole step --------------------------------------------------------------------------------------------------
STEP_CASES = [(16, 1, 1), (64, 1, 3)]          # (T, model seed, data seed): chosen with the oracle alone (see _step_case)
NFB, BATCH, MARGIN, DRP = 4, 3, 4, 0.05


@functools.lru_cache(maxsize=None)
def _step_case(T, mseed, dseed):
    w = ref.make_model(NFB, mseed, head_scale=1.0)
    x = ref.make_traces(BATCH, T, dseed)
    rs = np.random.RandomState(dseed)
    y = (rs.uniform(size=(BATCH, T)) < 0.15).astype(np.uint8)
    masks = tref.make_masks(NFB, BATCH, T, DRP, dseed)
    step = tref.TrainStep(w, MARGIN, DRP).run(x, y, masks)
    # the float64 network is away from every discontinuity: a ReLU gate, a pooling choice or a head-window argmax that fp32
    # rounding could flip would make the comparison meaningless
    assert min(step.margins) > 1e-5, step.margins
    return w, x, y, masks, step


@pytest.mark.parametrize('case', STEP_CASES, ids=lambda c: 'T%d' % c[0])
def test_train_step_against_the_oracle(dclib, case):
    from deep_calcium_amd.unet1d_train import UNet1DTrainEngine, metrics_from_sums
    T = case[0]
    w, x, y, masks, step = _step_case(*case)
    eng = UNet1DTrainEngine((T,), nb_filters_base=NFB, prop_dropout_base=DRP, margin=MARGIN)
    eng.set_weights(w)
    p = eng.forward_backward(x, y, masks).cpu().numpy()
    sums = eng.read_sums()
    g1 = eng.grads()
    after = eng.get_weights()
    loss = metrics_from_sums(sums, BATCH, T)[0]
    print('step T=%d: loss %.6f (oracle %.6f)  max |dp| %.3g  margins %r' % (T, loss, step.loss, np.abs(p - step.p).max(), step.margins))
    assert abs(loss - step.loss) <= 1e-4 * abs(step.loss) and np.abs(p - step.p).max() <= 1e-4
    worst = 0.
    for i in range(110):
        if i % 6 >= 4 and i < 108:                         # moving statistics: updated by the forward (momentum 0.99, biased variance)
            err = _rel(after[i], step.moving[i])
            assert err <= 1e-4, (i, err)
            continue
        assert np.array_equal(after[i], w[i])              # no parameter moved
        want = step.grads[i]
        scale = np.abs(want).max()
        if i % 6 == 1 and i < 108:
            # a conv bias in front of BatchNorm: its gradient, the sum of dz, is analytically zero and the float64 value is
            # rounding noise; the sum's terms have the size of the beta gradient's (the same sum before centring), so that is
            # the scale the fp32 sum is held to
            scale = max(scale, np.abs(step.grads[i + 2]).max())
        err = float(np.abs(g1[i] - want).max() / scale)
        worst = max(worst, err)
        assert err <= 1e-4, (i, err)
    print('step T=%d: worst gradient tensor error %.3g' % (T, worst))
    # the same step from the same state: bit-identical gradients
    eng.set_weights(w)
    eng.forward_backward(x, y, masks)
    g1b = eng.grads()
    assert all(np.array_equal(a, b) for a, b in zip(g1, g1b) if a is not None)
    # two Adam steps: the device's weights against the Keras-form Adam in float64 applied to the device's own gradients
    eng.set_weights(w)
    eng.train_on_batch(x, y, masks)
    ga = eng.grads()
    eng.train_on_batch(x, y, masks)
    gb = eng.grads()
    w2 = eng.get_weights()
    assert eng.iterations == 2
    for i in range(110):
        if i % 6 >= 4 and i < 108:
            continue
        p0 = np.asarray(w[i], np.float64)
        p1, m, v = tref.adam_keras(p0, ga[i].astype(np.float64), 0., 0., 0)
        p2, _, _ = tref.adam_keras(p1, gb[i].astype(np.float64), m, v, 1)
        # fp32 storage of two updates of size ~lr: 1e-4 of the update plus the rounding of the stored weight
        tol = 1e-4 * np.abs(p2 - p0).max() + 4 * 2. ** -24 * max(np.abs(p0).max(), 1e-3)
        assert np.abs(w2[i] - p2).max() <= tol, (i, np.abs(w2[i] - p2).max(), tol)


def test_train_engine_evaluate_and_predict_run_in_inference_mode(dclib):
    from deep_calcium_amd.unet1d_train import UNet1DTrainEngine
    T = 64
    w, x, y, masks, _ = _step_case(*STEP_CASES[1])
    eng = UNet1DTrainEngine((T,), nb_filters_base=NFB, prop_dropout_base=DRP, margin=MARGIN)
    eng.set_weights(w)
    p_want = ref.forward(w, x, MARGIN)
    p = eng.predict(x)
    assert np.abs(p - p_want).max() <= 1e-4
    got = eng.evaluate(x, y, batch_size=2)                # two batches (2 + 1 windows), sample-weighted
    want = np.zeros(6)
    for a in (0, 2):
        pw, yw = p_want[a:a + 2], y[a:a + 2]
        s = np.concatenate([[tref.loss_np(pw, yw) * pw.size], tref.metric_sums(pw, yw)])
        from deep_calcium_amd.unet1d_train import metrics_from_sums
        want += len(pw) * np.asarray(metrics_from_sums(s, len(pw), T))
    want /= BATCH
    print('evaluate: %r (oracle %r)' % (got, list(want)))
    assert np.abs(np.asarray(got) - want).max() <= 1e-4 * max(np.abs(want).max(), 1.)
    eng.train_on_batch(x, y, masks)                       # the weights moved: the inference engine is rebuilt
    assert np.abs(eng.predict(x) - ref.forward(eng.get_weights(), x, MARGIN)).max() <= 1e-4


# ---- fit() end to end ------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def spike_datasets(tmp_path_factory):
    """Two dataset files of 6 traces x 96 frames: sparse binary spikes, the trace a decaying bump after each spike plus noise."""
    from deep_calcium_amd.traces import write_traces_dataset
    d = tmp_path_factory.mktemp('spike_ds')
    rs = np.random.RandomState(42)
    paths = []
    for k in range(2):
        sp = (rs.uniform(size=(6, 96)) < 0.06).astype(np.uint8)
        tr = 0.2 * rs.randn(6, 96)
        for r, t in zip(*np.nonzero(sp)):
            n = min(8, 96 - t)
            tr[r, t:t + n] += 3. * np.exp(-np.arange(n) / 3.)
        paths.append(write_traces_dataset(str(d / ('ds%d.hdf5' % k)), tr.astype(np.float32) * 100 + 500, 'ds%d' % k, spikes=sp))
    return paths


def _builder_nfb4(window_shape, margin=4):
    from deep_calcium_amd.unet1d_train import UNet1DTrainEngine
    return UNet1DTrainEngine(window_shape, nb_filters_base=4, prop_dropout_base=0., margin=margin)


@pytest.mark.parametrize('val_type', ['random_split', 'cross_validate'])
def test_fit_end_to_end(dclib, spike_datasets, tmp_path, val_type):
    from deep_calcium_amd import TrainableUNet1DSegmentation, UNet1DSegmentation
    from deep_calcium_amd.keras_io import read_keras_unet1d
    np.random.seed(7)
    model = TrainableUNet1DSegmentation(str(tmp_path / 'cp'), net_builder_func=_builder_nfb4)
    # three epochs of two or three steps: with Adam's first steps of size lr per parameter, lr = 0.002 moves a kernel weight (std 0.3
    # at nfb 4) by at most 0.018 in all and the loss trend would be of the size of the batch-to-batch scatter of 4 x 64 samples;
    # lr = 0.01 makes the trend the larger of the two, so "the loss went down" tests the training and not the sampler
    from deep_calcium_amd import Adam
    history, best = model.fit(spike_datasets, shape=(64,), error_margin=2., batch=4, nb_epochs=3, val_type=val_type, nb_folds=2,
                              optimizer=Adam(0.01))
    histories = history if val_type == 'cross_validate' else [history]
    assert len(histories) == (2 if val_type == 'cross_validate' else 1)
    names = ['loss', 'F2', 'prec', 'reca', 'ytspks', 'ypspks']
    for h in histories:
        assert set(h) == set(names + ['val_' + n for n in names])
        assert all(len(v) == 3 and np.all(np.isfinite(v)) for v in h.values())
        print('fit %s: loss per epoch %r, val_F2 %r' % (val_type, h['loss'], h['val_F2']))
        assert h['loss'][-1] < h['loss'][0]                  # fixed seeds, dropout 0: three epochs of Adam(0.002) lower the loss
    csvs = [f for f in os.listdir(model.cpdir) if f.endswith('_metrics.csv')]
    assert len(csvs) == len(histories)
    assert open(os.path.join(model.cpdir, csvs[0])).readline().startswith('epoch,')
    mt = model.metrics_trn if val_type == 'random_split' else model.metrics_trn[0]
    assert set(mt) == set(names) and np.all(np.isfinite(list(mt.values())))
    assert os.path.isfile(best) and os.path.dirname(best) == model.cpdir and '_model_val_F2_' in os.path.basename(best)
    assert read_keras_unet1d(best)['config']['margin'] == 2 and read_keras_unet1d(best)['config']['nb_filters_base'] == 4
    spikes, dsnames = UNet1DSegmentation(str(tmp_path / 'cp2')).predict(spike_datasets[:1], best)
    assert dsnames == ['ds0'] and spikes[0].shape == (6, 96) and spikes[0].dtype == np.uint8


def test_example_train_sub_command(spike_datasets, tmp_path):
    """examples/spikes/unet1d.py train in a child process: it prints and writes the best model's path, which predict() reads."""
    from deep_calcium_amd import UNet1DSegmentation
    cp = str(tmp_path / 'cp')
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'spikes', 'unet1d.py'), 'train', ','.join(spike_datasets), '-c', cp,
                          '--shape', '64', '--batch', '4', '--epochs', '1', '--nb_filters_base', '4', '--seed', '3'],
                         capture_output=True, text=True, timeout=300, env=dict(os.environ, PYTHONPATH=ROOT))
    assert out.returncode == 0, out.stderr[-2000:]
    best = open(os.path.join(cp, 'best_model.txt')).read().strip()
    assert best == out.stdout.strip().splitlines()[-1] and os.path.isfile(best)
    spikes, _ = UNet1DSegmentation(cp).predict(spike_datasets, best)
    assert [s.shape for s in spikes] == [(6, 96), (6, 96)]
