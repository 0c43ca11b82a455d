"""The multi-tile loops of the persistent kernels against the float64 numpy oracle at ragged shapes, through the C ABI.

Every hot convolution kernel walks SEVERAL pixel tiles per workgroup in production (a 512^2 x 16 step: 64 tiles per
weight-gradient workgroup), the next tile's operands in flight while the current one is computed; the direct tests of
test_hip_ops.py / test_dzin_gpu.py run them at ONE tile per workgroup almost everywhere.  This module enters those loops:

  * weight gradients (wgrad_f16x3.hip, every instantiation of both dispatch macros, wgrad.hip, conv_c1.hip): 2 / 3 / 4 / 5
    tiles per workgroup, short last split, ragged tiles, ranges that cross an image boundary, ragged channel blocks
    (case tables + their proof on the CPU: tests/_tileplan.py, tests/test_tileplan.py);
  * the role-split kernel (igemm_pp.hip, every variant, both instantiations) and the joint backward kernels
    (bwd_joint.hip): item counts strictly between k and k + 1 times the CU count and no multiple of 8 -- n and n + 1 items
    per workgroup side by side, an uneven split over the XCDs -- with H and W both ragged.  The batch size is derived from
    the device's CU count.

Input construction, references and tolerances are the single-tile tests' (2e-5 of the output's maximum for the contractions;
the statistics / BatchNorm-sum bounds of the tests named at each assertion); outputs are prefilled with NaN; every
launch pair must be bit-equal (fixed-order reductions)."""
import numpy as np
import pytest

import _tileplan as tp
from oracle import unet_numpy as on

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import test_dzin_gpu as _dz          # noqa: E402  the dz-on-load input construction (values off the ReLU gate: the device's own gate)

dev, _block_case, _dz_ref, _finalize = _dz.dev, _dz._block_case, _dz._dz_ref, _dz._finalize
TOL = 2e-5


@pytest.fixture(autouse=True)
def _keep_alive():
    yield
    torch.cuda.synchronize()
    del _dz._KEEP[:]


def rel_err(got, ref):
    got = np.asarray(got.cpu().numpy() if hasattr(got, 'cpu') else got, np.float64)
    assert np.isfinite(got).all(), 'elements never written / not finite: %d' % int((~np.isfinite(got)).sum())
    return float(np.abs(got - ref).max() / np.abs(ref).max())


def nan(*shape, dtype=None):
    return torch.full(shape, float('nan'), device='cuda', dtype=dtype or torch.float32)


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def pow2_scale(L, a):
    scl = torch.empty(4, device='cuda')
    L.dc_pow2_scale_from_absmax(dev(np.array([np.abs(a).max()], np.float32)).data_ptr(), 1, 1024.0, scl.data_ptr(), None)
    _dz._KEEP.append(scl)
    return scl


def twice(launch, *shape):
    """Two launches into separate NaN-filled buffers: bit-equal, no tolerance.  Returns the first."""
    a, b = nan(*shape), nan(*shape)
    launch(a)
    launch(b)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not torch.isnan(a).any(), 'not bit-reproducible / not fully written'
    return a


def _case_id(c):
    return '%s-%s-%dt' % (c[0], c[1], c[7])


# ------------------------------------------------------------------------------------------------------ weight gradients
@pytest.mark.parametrize('case', tp.WGRAD_CASES, ids=_case_id)
def test_conv3x3_wgrad_multitile(dclib, case):
    """Every conv3x3 weight-gradient entry point at 2 / 3 / 4 / 5 tiles per workgroup (tests/_tileplan.py WGRAD_CASES): plain
    (gradient-sized dz + dz_scale), BN + ReLU on load, dz on load without and with in_scale (the 32-wide-tile instantiations
    take the one-(da, z)-set pipeline there), and the fp32 kernel on the plain data -- each against the float64 oracle at 2e-5,
    each launched twice, bit-equal."""
    L = dclib
    kind, inst, N, H, W, Ci, Co, tps, last = case
    # the mirror against the library: instantiation and tile shape from the kernel's name, split count from the workspace
    TW, TH, CM, CN, total, got_tps, splits, got_last = tp.wgrad_plan(kind, N, H, W, Ci, Co)
    for dzin in (0, 1):
        name = L.dc_conv3x3_wgrad_kernel_name(N, H, W, Ci, Co, dzin).decode()
        assert name == tp.wgrad_kernel_name(kind, W, Ci, Co, bool(dzin)), (case, name)
        tw, rw, wm, wnw, nbw = (int(v) for v in name.split('<')[1].split(',')[4:9])
        assert (tw, 4 // (wm * wnw) * rw, 32 * wm, 32 * wnw * nbw) == (TW, TH, CM, CN), (case, name)
    assert (got_tps, got_last) == (tps, last), case
    ws_floats = L.dc_conv3x3_wgrad_ws_floats(N, H, W, Ci, Co)
    assert ws_floats >= (splits + 32) * 9 * Ci * Co, (case, ws_floats, splits)

    rs = np.random.RandomState(N * 1000 + H * 7 + W + Ci)
    x, z, mean, invstd, gamma, beta, da = _block_case(rs, N, H, W, Ci, Co)
    dz_ref, _, _, _ = _dz_ref(z, mean, invstd, gamma, beta, da)
    dz = (rs.standard_normal((N, H, W, Co)) * 3e-7).astype(np.float32)              # gradient magnitudes, as test_hip_ops.py
    xsc = (rs.random_sample(Ci) + 0.5).astype(np.float32); xsh = (rs.standard_normal(Ci) * 0.3).astype(np.float32)
    x64 = x.astype(np.float64)
    x_eff = np.maximum(x64 * xsc.astype(np.float64) + xsh.astype(np.float64), 0.0)
    K0 = np.zeros((3, 3, Ci, Co))
    ref = {(a, b): on.conv3x3_bwd(xv, K0, dv)[1] for a, xv in (('x', x64), ('bn', x_eff))
           for b, dv in (('dz', dz.astype(np.float64)), ('dzin', dz_ref))}

    zd, dad, coef, _, _, _ = _finalize(L, z, mean, invstd, gamma, beta, da)
    xd, dzd, scd, shd = dev(x), dev(dz), dev(xsc), dev(xsh)
    scl = pow2_scale(L, dz)
    ws = torch.empty(ws_floats, device='cuda')
    shape = (3, 3, Ci, Co)
    got = {
        'f16x3': (twice(lambda o: L.dc_conv3x3_wgrad_f16x3(xd.data_ptr(), dzd.data_ptr(), o.data_ptr(), ws.data_ptr(), scl.data_ptr(), None,
                                                            N, H, W, Ci, Co, None), *shape), ref['x', 'dz']),
        'bnin': (twice(lambda o: L.dc_conv3x3_wgrad_bnin_f16x3(xd.data_ptr(), scd.data_ptr(), shd.data_ptr(), None, dzd.data_ptr(), o.data_ptr(),
                                                                ws.data_ptr(), scl.data_ptr(), N, H, W, Ci, Co, None), *shape), ref['bn', 'dz']),
        'dzin': (twice(lambda o: L.dc_conv3x3_wgrad_dzin_f16x3(xd.data_ptr(), None, None, None, dad.data_ptr(), zd.data_ptr(), coef.data_ptr(),
                                                                o.data_ptr(), ws.data_ptr(), N, H, W, Ci, Co, None), *shape), ref['x', 'dzin']),
        'dzin+in_scale': (twice(lambda o: L.dc_conv3x3_wgrad_dzin_f16x3(xd.data_ptr(), scd.data_ptr(), shd.data_ptr(), None, dad.data_ptr(),
                                                                         zd.data_ptr(), coef.data_ptr(), o.data_ptr(), ws.data_ptr(),
                                                                         N, H, W, Ci, Co, None), *shape), ref['bn', 'dzin']),
        'fp32': (twice(lambda o: L.dc_conv3x3_wgrad(xd.data_ptr(), dzd.data_ptr(), o.data_ptr(), ws.data_ptr(), N, H, W, Ci, Co, None), *shape),
                 ref['x', 'dz']),
    }
    errs = {k: rel_err(g, r) for k, (g, r) in got.items()}
    print('wgrad %s: %s' % (_case_id(case), ' '.join('%s %.2e' % kv for kv in errs.items())))
    assert all(e < TOL for e in errs.values()), (case, errs)


@pytest.mark.parametrize('case', tp.CONVT_WGRAD_CASES, ids=_case_id)
def test_convT2x2_wgrad_multitile(dclib, case):
    """The conv-transpose weight-gradient entry points (split-fp16 plain and BN + ReLU on load, fp32) at 2 / 3 / 4 / 5 tiles per
    workgroup (CONVT_WGRAD_CASES) against the float64 oracle at 2e-5; each launched twice, bit-equal."""
    L = dclib
    kind, inst, N, H, W, Ci, Co, tps, last = case
    TW, TH, CM, CN, total, got_tps, splits, got_last = tp.wgrad_plan(kind, N, H, W, Ci, Co)
    assert (got_tps, got_last) == (tps, last), case
    ws_floats = L.dc_convT2x2_wgrad_ws_floats(N, H, W, Ci, Co)
    assert ws_floats >= (splits + 32) * 4 * Ci * Co, (case, ws_floats, splits)
    rs = np.random.RandomState(N * 1000 + H * 7 + W + Ci)
    x = rs.standard_normal((N, H, W, Ci)).astype(np.float32)
    dz = (rs.standard_normal((N, 2 * H, 2 * W, Co)) * 1e-7).astype(np.float32)
    xsc = (rs.random_sample(Ci) + 0.5).astype(np.float32); xsh = (rs.standard_normal(Ci) * 0.3).astype(np.float32)
    x64 = x.astype(np.float64)
    x_eff = np.maximum(x64 * xsc.astype(np.float64) + xsh.astype(np.float64), 0.0)
    K0 = np.zeros((2, 2, Co, Ci))
    ref_x = on.convT2x2_bwd(x64, K0, dz.astype(np.float64))[1]
    ref_bn = on.convT2x2_bwd(x_eff, K0, dz.astype(np.float64))[1]
    xd, dzd, scd, shd = dev(x), dev(dz), dev(xsc), dev(xsh)
    scl = pow2_scale(L, dz)
    ws = torch.empty(ws_floats, device='cuda')
    shape = (2, 2, Co, Ci)
    got = {
        'f16x3': (twice(lambda o: L.dc_convT2x2_wgrad_f16x3(xd.data_ptr(), dzd.data_ptr(), o.data_ptr(), ws.data_ptr(), scl.data_ptr(), None,
                                                             N, H, W, Ci, Co, None), *shape), ref_x),
        'bnin': (twice(lambda o: L.dc_convT2x2_wgrad_bnin_f16x3(xd.data_ptr(), scd.data_ptr(), shd.data_ptr(), None, dzd.data_ptr(), o.data_ptr(),
                                                                 ws.data_ptr(), scl.data_ptr(), N, H, W, Ci, Co, None), *shape), ref_bn),
        'fp32': (twice(lambda o: L.dc_convT2x2_wgrad(xd.data_ptr(), dzd.data_ptr(), o.data_ptr(), ws.data_ptr(), N, H, W, Ci, Co, None), *shape),
                 ref_x),
    }
    errs = {k: rel_err(g, r) for k, (g, r) in got.items()}
    print('convT wgrad %s: %s' % (_case_id(case), ' '.join('%s %.2e' % kv for kv in errs.items())))
    assert all(e < TOL for e in errs.values()), (case, errs)


@pytest.mark.parametrize('N,H,W,Co,trips', tp.C1_WGRAD_CASES)
def test_first_layer_wgrad_multitrip(dclib, N, H, W, Co, trips):
    """Cin == 1 (conv_c1.hip): more pixels than 2048 blocks take in one trip, so the grid-stride loop of both kernels (W % 4 == 0 and
    the generic one) runs more than once per workgroup; plain and dz on load against the float64 oracle."""
    L = dclib
    assert tp.c1_plan(N, H, W, Co) == (2048, trips)
    assert L.dc_conv3x3_wgrad_ws_floats(N, H, W, 1, Co) == (2048 + 32) * 9 * Co
    rs = np.random.RandomState(W + Co)
    _, z, mean, invstd, gamma, beta, da = _block_case(rs, N, H, W, 4, Co)
    x = rs.standard_normal((N, H, W, 1)).astype(np.float32)
    dz = rs.standard_normal((N, H, W, Co)).astype(np.float32)
    dz_ref, _, _, _ = _dz_ref(z, mean, invstd, gamma, beta, da)
    K0 = np.zeros((3, 3, 1, Co))
    ref_plain = on.conv3x3_bwd(x.astype(np.float64), K0, dz.astype(np.float64))[1]
    ref_dzin = on.conv3x3_bwd(x.astype(np.float64), K0, dz_ref)[1]
    zd, dad, coef, _, _, _ = _finalize(L, z, mean, invstd, gamma, beta, da)
    xd, dzd = dev(x.reshape(N, H, W)), dev(dz)
    ws = torch.empty(L.dc_conv3x3_wgrad_ws_floats(N, H, W, 1, Co), device='cuda')
    shape = (3, 3, 1, Co)
    g_plain = twice(lambda o: L.dc_conv3x3_wgrad(xd.data_ptr(), dzd.data_ptr(), o.data_ptr(), ws.data_ptr(), N, H, W, 1, Co, None), *shape)
    g_dzin = twice(lambda o: L.dc_conv3x3_wgrad_dzin_f16x3(xd.data_ptr(), None, None, None, dad.data_ptr(), zd.data_ptr(), coef.data_ptr(),
                                                           o.data_ptr(), ws.data_ptr(), N, H, W, 1, Co, None), *shape)
    e1, e2 = rel_err(g_plain, ref_plain), rel_err(g_dzin, ref_dzin)
    print('first layer wgrad (%d,%d,%d,%d): plain %.2e dzin %.2e' % (N, H, W, Co, e1, e2))
    assert e1 < TOL and e2 < TOL, (e1, e2)


# ---------------------------------------------------------------------------------- role-split kernel and joint backward
# H, W: both ragged for the instantiation's tile (8 x 32 / 16 x 32), W > 32, even (the pooled variant); the batch size comes from
# the device's CU count.  (Cin, Cout) are the LAYER's: the GEMM columns are Cout forward, Cin for the data gradients.
PP_FWD = {'<2,2>': (12, 40, 64, 160), '<4,1>': (20, 40, 64, 32)}       # 3 column blocks, the last one half full / 1 column block
PP_FWD_WG = {'<2,2>': (12, 40, 64, 64), '<4,1>': (20, 40, 64, 32)}      # 1 column block: per-workgroup moments need tiles > 2 x #CUs
PP_DGRAD = {'<2,2>': (12, 40, 160, 64), '<4,1>': (20, 40, 32, 64)}
JOINT_HW = (10, 40)


def _family(k, H, W, Ncols, what):
    """N for this device, with every property of the family asserted through the mirror."""
    n_cus = cus()
    found = tp.persistent_family(k, n_cus, H, W, Ncols)
    assert found is not None, '%s: no batch size puts the item count between %d and %d x %d CUs' % (what, k, k + 1, n_cus)
    N, items = found
    th, tw = (tp.pp_tile(Ncols)[:2] if Ncols else (4, 32))
    assert N >= 2 and k * n_cus < items < (k + 1) * n_cus and items % 8 != 0, (what, N, items)
    assert H % th != 0 and W % tw != 0 and W > 32, (what, H, W)
    plan = tp.persistent_plan(items, n_cus)
    assert len(plan) == n_cus and {len(wg) for wg in plan} == {k, k + 1}, what
    return N, items


def _conv_inputs(rs, N, H, W, Ci, Co, bias_sigmas=0):
    x = rs.standard_normal((N, H, W, Ci)).astype(np.float32)
    K = (rs.standard_normal((3, 3, Ci, Co)) * np.sqrt(2.0 / (9 * Ci))).astype(np.float32)
    b = (rs.standard_normal(Co) + bias_sigmas * np.sqrt(2.0)).astype(np.float32)
    return x, K, b


def _pack_fwd(L, K, Ci, Co):
    wp = torch.empty(L.dc_pack_weights_f16x3_floats(9, Ci, Co), device='cuda')
    L.dc_pack_weights_f16x3(dev(K).data_ptr(), wp.data_ptr(), 9, Ci, Co, Ci * Co, Co, 1, 0, None)
    _dz._KEEP.append(wp)
    return wp


def _pack_dgrad(L, K, Ci, Co):
    wpd = torch.empty(L.dc_pack_weights_f16x3_floats(9, Co, Ci), device='cuda')
    L.dc_pack_weights_f16x3(dev(K).data_ptr(), wpd.data_ptr(), 9, Co, Ci, Ci * Co, 1, Co, 1, None)
    _dz._KEEP.append(wpd)
    return wpd


def _finalize_stats(L, st, rows, Co, count):
    mean, invstd = torch.empty(Co, device='cuda'), torch.empty(Co, device='cuda')
    L.dc_bn_stats_finalize(st.data_ptr(), rows, 1, Co, float(count), 1e-3, -1.0, mean.data_ptr(), invstd.data_ptr(), None, None, None)
    torch.cuda.synchronize()
    return mean.cpu().numpy().astype(np.float64), invstd.cpu().numpy().astype(np.float64)


def _check_moments(mean, invstd, z_dev):
    """The bounds of test_conv3x3_bn_partials_per_workgroup, against a float64 reduction of the z the kernel wrote."""
    zr = z_dev.cpu().numpy().astype(np.float64).reshape(-1, z_dev.shape[-1])
    mu, var = zr.mean(0), zr.var(0)
    assert np.abs(mean - mu).max() < 2e-6 * np.abs(mu).max() + 1e-6 * np.sqrt(var).max()
    assert np.abs(invstd * np.sqrt(var + 1e-3) - 1).max() < 2e-5


@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('inst', ['<2,2>', '<4,1>'])
def test_pp_forward_uneven_items(dclib, inst, k):
    """dc_conv3x3_fwd_f16x3 with one BatchNorm-partial row per tile: z and the finalized statistics against float64."""
    L = dclib
    H, W, Ci, Co = PP_FWD[inst]
    N, items = _family(k, H, W, Co, 'forward %s k=%d' % (inst, k))
    tiles = L.dc_conv3x3_tiles(N, H, W, Co)
    assert L.dc_conv3x3_pp_blocks(N, H, W, Ci, Co, 0, 1) == tp.pp_tiles(N, H, W, Co) == tiles, (inst, k, N)
    rs = np.random.RandomState(N + H + Co)
    x, K, b = _conv_inputs(rs, N, H, W, Ci, Co)
    z_ref = on.conv3x3_fwd(x.astype(np.float64), K.astype(np.float64), b.astype(np.float64))
    xd, bd, wp = dev(x), dev(b), _pack_fwd(L, K, Ci, Co)

    def run():
        z = nan(N, H, W, Co)
        st = nan(tiles * Co * 2, dtype=torch.float64)
        L.dc_conv3x3_fwd_f16x3(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), z.data_ptr(), Co, st.data_ptr(), 0, None, None, 0,
                               None, 0, None, 0, None, N, H, W, Ci, Co, None)
        torch.cuda.synchronize()
        return z, st

    z, st = run()
    z2, st2 = run()
    assert torch.equal(z, z2) and torch.equal(st, st2) and torch.isfinite(st).all()
    e = rel_err(z, z_ref)
    print('forward %s k=%d N=%d items=%d: z %.2e' % (inst, k, N, items, e))
    assert e < TOL
    s = st.cpu().numpy().reshape(tiles, Co, 2).sum(0)                                           # test_conv3x3_f16x3_fwd_dgrad's bounds
    assert np.allclose(s[:, 0], z_ref.sum((0, 1, 2)), rtol=1e-4, atol=1e-3 * np.sqrt(N * H * W))
    assert np.allclose(s[:, 1], (z_ref ** 2).sum((0, 1, 2)), rtol=1e-4)
    _check_moments(*_finalize_stats(L, st, tiles, Co, N * H * W), z)


@pytest.mark.parametrize('bias_sigmas', [0, 1000])
@pytest.mark.parametrize('inst', ['<2,2>', '<4,1>'])
def test_pp_forward_per_workgroup_moments_uneven_items(dclib, inst, bias_sigmas):
    """stats_rows = dc_conv3x3_stats_rows(): each (workgroup, consumer set) Chan-merges the tiles it walks -- 3 for some workgroups,
    4 for others, ragged ones among them -- into ONE row.  z bit-equal to the per-tile launch and to the oracle at 2e-5; the finalized
    mean / 1/std against float64, also at |mean| = 1000 sigma.  (The library uses per-workgroup rows only where they are fewer than the
    tiles, i.e. above 2 items per workgroup and with one column block: k = 3.)"""
    L = dclib
    H, W, Ci, Co = PP_FWD_WG[inst]
    N, items = _family(3, H, W, Co, 'per-workgroup moments %s' % inst)
    tiles, rows = L.dc_conv3x3_tiles(N, H, W, Co), L.dc_conv3x3_stats_rows(N, H, W, Ci, Co)
    assert L.dc_conv3x3_pp_blocks(N, H, W, Ci, Co, 0, 1) == tp.pp_tiles(N, H, W, Co) == tiles == items, (inst, N)
    assert rows == 2 * min(items, cus()) < tiles, (inst, N, rows, tiles)
    rs = np.random.RandomState(N + W + Co)
    x, K, b = _conv_inputs(rs, N, H, W, Ci, Co, bias_sigmas)
    z_ref = on.conv3x3_fwd(x.astype(np.float64), K.astype(np.float64), b.astype(np.float64))
    xd, bd, wp = dev(x), dev(b), _pack_fwd(L, K, Ci, Co)

    def run(stats_rows):
        z = nan(N, H, W, Co)
        n = stats_rows if stats_rows else tiles
        st = nan(n * Co * 2, dtype=torch.float64)
        L.dc_conv3x3_fwd_f16x3(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), z.data_ptr(), Co, st.data_ptr(), stats_rows, None, None, 0,
                               None, 0, None, 0, None, N, H, W, Ci, Co, None)
        torch.cuda.synchronize()
        assert torch.isfinite(st).all(), 'rows never written: %d' % int((~torch.isfinite(st)).sum())
        return z, st, n

    z0, st0, n0 = run(0)
    z1, st1, n1 = run(rows)
    z2, st2, _ = run(rows)
    assert torch.equal(z0, z1) and torch.equal(z1, z2) and torch.equal(st1, st2)
    e = rel_err(z1, z_ref)
    print('per-workgroup moments %s N=%d items=%d rows=%d mean=%d sigma: z %.2e' % (inst, N, items, rows, bias_sigmas, e))
    assert e < TOL
    _check_moments(*_finalize_stats(L, st1, n1, Co, N * H * W), z1)
    _check_moments(*_finalize_stats(L, st0, n0, Co, N * H * W), z0)


@pytest.mark.parametrize('inst', ['<2,2>', '<4,1>'])
def test_pp_forward_bnin_uneven_items(dclib, inst):
    """dc_conv3x3_fwd_bnin_f16x3: relu(fmaf(z_in, sc, sh)) formed while staging, zero padding kept zero (positive shifts), against the
    float64 oracle on the float64 activation."""
    L = dclib
    H, W, Ci, Co = PP_FWD[inst]
    N, items = _family(1, H, W, Co, 'forward bnin %s' % inst)
    assert L.dc_conv3x3_pp_blocks(N, H, W, Ci, Co, 0, 0) == tp.pp_tiles(N, H, W, Co), (inst, N)
    rs = np.random.RandomState(N * 77 + H + Ci)
    zin = (rs.standard_normal((N, H, W, Ci)) * 2 + 0.5).astype(np.float32)
    _, K, b = _conv_inputs(rs, N, H, W, Ci, Co)
    sc = (rs.random_sample(Ci) + 0.5).astype(np.float32); sh = (rs.standard_normal(Ci) * 0.5 + 0.3).astype(np.float32)     # mostly positive shifts
    a_ref = np.maximum(zin.astype(np.float64) * sc.astype(np.float64) + sh.astype(np.float64), 0.0)
    z_ref = on.conv3x3_fwd(a_ref, K.astype(np.float64), b.astype(np.float64))
    zind, scd, shd, bd, wp = dev(zin), dev(sc), dev(sh), dev(b), _pack_fwd(L, K, Ci, Co)
    z = twice(lambda o: L.dc_conv3x3_fwd_bnin_f16x3(zind.data_ptr(), scd.data_ptr(), shd.data_ptr(), None, wp.data_ptr(), bd.data_ptr(),
                                                    o.data_ptr(), Co, None, 0, None, None, 0, None, N, H, W, Ci, Co, None), N, H, W, Co)
    e = rel_err(z, z_ref)
    print('forward bnin %s N=%d items=%d: z %.2e' % (inst, N, items, e))
    assert e < TOL


@pytest.mark.parametrize('inst', ['<2,2>', '<4,1>'])
def test_pp_forward_pool_uneven_items(dclib, inst):
    """dc_conv3x3_fwd_pool_f16x3 (folded BN + ReLU): its z against the oracle, its pooled output bit-equal to dc_maxpool2x2_fwd of its
    own (strided) z."""
    L = dclib
    H, W, Ci, Co = PP_FWD[inst]
    N, items = _family(1, H, W, Co, 'forward pool %s' % inst)
    assert L.dc_conv3x3_fwd_pool_blocks(N, H, W, Ci, Co) == tp.pp_tiles(N, H, W, Co), (inst, N)
    rs = np.random.RandomState(H + Co)
    x, K, b = _conv_inputs(rs, N, H, W, Ci, Co)
    sc = (rs.random_sample(Co) + 0.5).astype(np.float32); sh = (rs.standard_normal(Co) * 0.4).astype(np.float32)
    z_ref = on.conv3x3_fwd(x.astype(np.float64), K.astype(np.float64), b.astype(np.float64))
    a_ref = np.maximum(z_ref * sc.astype(np.float64) + sh.astype(np.float64), 0.0)
    xd, bd, scd, shd, wp = dev(x), dev(b), dev(sc), dev(sh), _pack_fwd(L, K, Ci, Co)
    ld = 2 * Co

    def run():
        cat = torch.zeros((N, H, W, ld), device='cuda')
        cat[..., Co:] = float('nan')
        pool = nan(N, H // 2, W // 2, Co)
        flag = torch.zeros(4, device='cuda')
        L.dc_conv3x3_fwd_pool_f16x3(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), cat.data_ptr() + 4 * Co, ld, scd.data_ptr(), shd.data_ptr(), 1,
                                    flag.data_ptr(), pool.data_ptr(), N, H, W, Ci, Co, None)
        torch.cuda.synchronize()
        return cat, pool

    cat, pool = run()
    cat2, pool2 = run()
    assert torch.equal(cat, cat2) and torch.equal(pool, pool2)
    assert (cat[..., :Co] == 0).all()
    e = rel_err(cat[..., Co:], a_ref)
    print('forward pool %s N=%d items=%d: activation %.2e' % (inst, N, items, e))
    assert e < TOL
    own = nan(N, H // 2, W // 2, Co)
    L.dc_maxpool2x2_fwd(cat.data_ptr() + 4 * Co, ld, own.data_ptr(), None, N, H, W, Co, None)
    torch.cuda.synchronize()
    assert torch.equal(pool, own) and torch.isfinite(pool).all() and (pool > 0).any()


def _bn_red_reference(dx_dev, rz, rmu, ris, rga, rbe):
    """float64 pass-1 sums / max |dy| of the layer in front from the dx the kernel wrote (test_conv3x3_dgrad_dzin)."""
    Cin = rz.shape[-1]
    sc = (rga * ris).astype(np.float32)
    sh = (rbe.astype(np.float64) - rmu.astype(np.float64) * sc.astype(np.float64)).astype(np.float32)
    za = rz.astype(np.float64).reshape(-1, Cin)
    gate = (za * sc.astype(np.float64) + sh.astype(np.float64)) > 0
    dy = np.where(gate, dx_dev.cpu().numpy().astype(np.float64).reshape(-1, Cin), 0.0)
    return dy.sum(0), (dy * (za - rmu.astype(np.float64)) * ris.astype(np.float64)).sum(0), np.abs(dy).max(0).astype(np.float32)


def _check_bn_red(L, part, amx, rows, Cin, dx_dev, red_np):
    assert torch.isfinite(part).all() and torch.isfinite(amx).all(), 'partial rows never written'
    dg, db = torch.zeros(Cin, device='cuda'), torch.zeros(Cin, device='cuda')
    L.dc_bn_bwd_finalize(part.data_ptr(), rows, Cin, dg.data_ptr(), db.data_ptr(), None)
    torch.cuda.synchronize()
    ref_db, ref_dg, ref_amax = _bn_red_reference(dx_dev, *red_np)
    tol = 2e-5 * max(np.abs(ref_dg).max(), np.abs(ref_db).max())
    assert np.abs(dg.cpu().numpy() - ref_dg).max() < tol and np.abs(db.cpu().numpy() - ref_db).max() < tol
    assert np.array_equal(amx.cpu().numpy().reshape(rows, Cin).max(0), ref_amax)


def _red_layer(rs, N, H, W, Cin):
    rz = rs.standard_normal((N, H, W, Cin)).astype(np.float32)
    rmu = (rs.standard_normal(Cin) * 0.2).astype(np.float32); ris = (rs.random_sample(Cin) + 0.5).astype(np.float32)
    rga = rs.standard_normal(Cin).astype(np.float32); rbe = (rs.standard_normal(Cin) * 0.3).astype(np.float32)
    return rz, rmu, ris, rga, rbe


@pytest.mark.parametrize('k', [1, 3])
@pytest.mark.parametrize('inst', ['<2,2>', '<4,1>'])
def test_pp_dgrad_uneven_items(dclib, inst, k):
    """dc_conv3x3_dgrad_f16x3 (gradient-sized dz + power-of-two scale) against the float64 oracle; at k = 1 also
    dc_conv3x3_dgrad_bnred_f16x3: the same dx bit for bit, its sums and amax_partial against float64."""
    L = dclib
    H, W, Ci, Co = PP_DGRAD[inst]
    N, items = _family(k, H, W, Ci, 'dgrad %s k=%d' % (inst, k))
    assert L.dc_conv3x3_pp_blocks(N, H, W, Ci, Co, 1, 0) == tp.pp_tiles(N, H, W, Ci), (inst, k, N)
    rs = np.random.RandomState(N + Ci + H)
    dz = (rs.standard_normal((N, H, W, Co)) * 3e-7).astype(np.float32)
    K = (rs.standard_normal((3, 3, Ci, Co)) * 0.05).astype(np.float32)
    dx_ref, _, _ = on.conv3x3_bwd(np.zeros((N, H, W, Ci)), K.astype(np.float64), dz.astype(np.float64))
    dzd, wpd, scl = dev(dz), _pack_dgrad(L, K, Ci, Co), pow2_scale(L, dz)
    dx = twice(lambda o: L.dc_conv3x3_dgrad_f16x3(dzd.data_ptr(), wpd.data_ptr(), o.data_ptr(), scl.data_ptr(), None, 0, None,
                                                  N, H, W, Ci, Co, None), N, H, W, Ci)
    e = rel_err(dx, dx_ref)
    print('dgrad %s k=%d N=%d items=%d: dx %.2e' % (inst, k, N, items, e))
    assert e < TOL
    if k != 1:
        return
    rows = L.dc_conv3x3_dgrad_bnred_blocks(N, H, W, Ci, Co)
    assert rows == tp.pp_tiles(N, H, W, Ci), (inst, N, rows)
    red_np = _red_layer(rs, N, H, W, Ci)
    red = [dev(a) for a in red_np]

    def run():
        o, part, amx = nan(N, H, W, Ci), nan(rows * Ci * 2), nan(rows * Ci)
        L.dc_conv3x3_dgrad_bnred_f16x3(dzd.data_ptr(), wpd.data_ptr(), o.data_ptr(), scl.data_ptr(), None, 0, *[t.data_ptr() for t in red],
                                       part.data_ptr(), amx.data_ptr(), N, H, W, Ci, Co, None)
        torch.cuda.synchronize()
        return o, part, amx

    dx1, part, amx = run()
    dx2, part2, amx2 = run()
    assert torch.equal(dx1, dx) and torch.equal(dx1, dx2) and torch.equal(part, part2) and torch.equal(amx, amx2)
    _check_bn_red(L, part, amx, rows, Ci, dx1, red_np)


@pytest.mark.parametrize('inst,mode', [('<2,2>', 'plain'), ('<2,2>', 'red_z'), ('<2,2>', 'dz_out'), ('<4,1>', 'plain'), ('<4,1>', 'red_z')])
def test_pp_dgrad_dzin_uneven_items(dclib, inst, mode):
    """dc_conv3x3_dgrad_dzin_f16x3: dx from the dz formed on load against the float64 oracle on the float64 dz; with red_z the fused
    sums of the layer in front; with dz_out (the 64-column instantiation only: the library refuses it at 32 columns) the written dz
    against the oracle's, every pixel written exactly once (NaN prefill; only the first of the 3 column blocks of a tile stores), dx
    unchanged bit for bit."""
    L = dclib
    H, W, Ci, Co = PP_DGRAD[inst]
    N, items = _family(1, H, W, Ci, 'dgrad dzin %s' % inst)
    rows = L.dc_conv3x3_dgrad_dzin_blocks(N, H, W, Ci, Co)
    assert rows == tp.pp_tiles(N, H, W, Ci), (inst, N, rows)
    rs = np.random.RandomState(Ci + Co + H + len(mode))
    x, z, mean, invstd, gamma, beta, da = _block_case(rs, N, H, W, Ci, Co)
    K = (rs.standard_normal((3, 3, Ci, Co)) * 0.05).astype(np.float32)
    dz_ref, _, _, _ = _dz_ref(z, mean, invstd, gamma, beta, da)
    dx_ref, _, _ = on.conv3x3_bwd(x.astype(np.float64), K.astype(np.float64), dz_ref)
    zd, dad, coef, _, _, _ = _finalize(L, z, mean, invstd, gamma, beta, da)
    wpd = _pack_dgrad(L, K, Ci, Co)
    red_np = _red_layer(rs, N, H, W, Ci)
    red = [dev(a) for a in red_np]

    def run(with_red, with_dzo):
        o, part, amx = nan(N, H, W, Ci), nan(rows * Ci * 2), nan(rows * Ci)
        dzo = nan(N, H, W, Co)
        ra = tuple(t.data_ptr() for t in red) + (part.data_ptr(), amx.data_ptr()) if with_red else (None,) * 7
        L.dc_conv3x3_dgrad_dzin_f16x3(dad.data_ptr(), zd.data_ptr(), coef.data_ptr(), wpd.data_ptr(), o.data_ptr(),
                                      dzo.data_ptr() if with_dzo else None, *ra, N, H, W, Ci, Co, None)
        torch.cuda.synchronize()
        return o, part, amx, dzo

    a = run(mode == 'red_z', mode == 'dz_out')
    b = run(mode == 'red_z', mode == 'dz_out')
    assert torch.equal(a[0], b[0])
    e = rel_err(a[0], dx_ref)
    print('dgrad dzin %s %s N=%d items=%d: dx %.2e' % (inst, mode, N, items, e))
    assert e < TOL
    if mode == 'red_z':
        assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        _check_bn_red(L, a[1], a[2], rows, Ci, a[0], red_np)
    if mode == 'dz_out':
        plain = run(False, False)
        assert torch.equal(plain[0], a[0]) and torch.equal(a[3], b[3])
        got = a[3].cpu().numpy()
        assert np.isfinite(got).all(), 'pixels the write-back missed: %d' % int((~np.isfinite(got)).sum())
        assert np.abs(got - dz_ref).max() < 2e-6 * np.abs(dz_ref).max()                # test_dgrad_dzin_writes_dz_...'s bound


@pytest.mark.parametrize('k', [1, 2])
@pytest.mark.parametrize('Cin', [32, 64])
def test_bwd_joint_uneven_items(dclib, Cin, k):
    """dc_conv3x3_bwd_joint_f16x3, 32 -> 32 (BN + ReLU on load, fused sums of the layer in front) and 64 -> 32: dx and dW against the
    float64 oracle on the float64 dz, k and k + 1 tiles per workgroup, H % 4 and W % 32 ragged; bit-reproducible."""
    L = dclib
    Cout = 32
    H, W = JOINT_HW
    N, items = _family(k, H, W, None, 'joint %d->32 k=%d' % (Cin, k))
    rows = L.dc_conv3x3_bwd_joint_blocks(N, H, W, Cin, Cout)
    assert rows == 2 * min(tp.joint_items(N, H, W), cus()), (Cin, k, N, rows)
    bnin = Cin == 32
    rs = np.random.RandomState(H * 7 + W + Cin + k)
    x, z, mean, invstd, gamma, beta, da = _block_case(rs, N, H, W, Cin, Cout)
    K = (rs.standard_normal((3, 3, Cin, Cout)) * 0.05).astype(np.float32)
    dz_ref, _, _, _ = _dz_ref(z, mean, invstd, gamma, beta, da)
    rmu = (rs.standard_normal(Cin) * 0.2).astype(np.float32); ris = (rs.random_sample(Cin) + 0.5).astype(np.float32)
    rga = (rs.standard_normal(Cin) * 0.5 + 1.0).astype(np.float32); rbe = (rs.standard_normal(Cin) * 0.3).astype(np.float32)
    xsc = (rga * ris).astype(np.float32)
    xsh = (rbe.astype(np.float64) - rmu.astype(np.float64) * xsc.astype(np.float64)).astype(np.float32)
    x_eff = np.maximum(x.astype(np.float64) * xsc.astype(np.float64) + xsh.astype(np.float64), 0.0) if bnin else x.astype(np.float64)
    dx_ref, dK_ref, _ = on.conv3x3_bwd(x_eff, K.astype(np.float64), dz_ref)
    zd, dad, coef, _, _, _ = _finalize(L, z, mean, invstd, gamma, beta, da)
    xd, wpd = dev(x), _pack_dgrad(L, K, Cin, Cout)
    ws = torch.empty(L.dc_conv3x3_bwd_joint_ws_floats(N, H, W, Cin, Cout), device='cuda')
    rmud, risd, rgad, rbed, xscd, xshd = dev(rmu), dev(ris), dev(rga), dev(rbe), dev(xsc), dev(xsh)

    def run():
        dx, dw = nan(N, H, W, Cin), nan(3, 3, Cin, Cout)
        part, amx = nan(rows * Cin * 2), nan(rows * Cin)
        ra = (xd.data_ptr(), rmud.data_ptr(), risd.data_ptr(), rgad.data_ptr(), rbed.data_ptr(), part.data_ptr(), amx.data_ptr()) if bnin \
            else (None,) * 7
        L.dc_conv3x3_bwd_joint_f16x3(xd.data_ptr(), xscd.data_ptr() if bnin else None, xshd.data_ptr() if bnin else None, None,
                                     dad.data_ptr(), zd.data_ptr(), coef.data_ptr(), wpd.data_ptr(), dx.data_ptr(), *ra,
                                     dw.data_ptr(), ws.data_ptr(), N, H, W, Cin, Cout, None)
        torch.cuda.synchronize()
        return dx, dw, part, amx

    dx, dw, part, amx = run()
    dx2, dw2, part2, amx2 = run()
    assert torch.equal(dx, dx2) and torch.equal(dw, dw2)
    ex, ew = rel_err(dx, dx_ref), rel_err(dw, dK_ref)
    print('joint %d->32 k=%d N=%d items=%d: dx %.2e dW %.2e' % (Cin, k, N, items, ex, ew))
    assert ex < TOL and ew < TOL, (ex, ew)
    if bnin:
        assert torch.equal(part, part2) and torch.equal(amx, amx2)
        _check_bn_red(L, part, amx, rows, Cin, dx, (x, rmu, ris, rga, rbe))
