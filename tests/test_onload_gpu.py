"""Two full-resolution tensors of the level-0 backward that their consumer rebuilds instead of reading (include/dcunet.h):

  * the head's activation gradient da = dlogits.Kh^T (Conv2D(2,1,softmax) of /root/reference/deepcalcium/models/neurons/
    unet_2d_summary.py:221-222) has rank one, da[pix][c] = kd[c] * s[pix]: dc_head_fwd_bwd_s / dc_head_bwd_bnin_bnred_s write the
    per-pixel factor s, dc_conv3x3_bwd_joint_r1_f16x3 forms the product on load;
  * the first layer's pre-BN output z (:170-172) is rebuilt by dc_conv3x3_c1_wgrad_dzin_zre from the image window it holds.

Both are exact by construction, so every comparison here is torch.equal against the EXISTING entry point on the same inputs (whose
float64-oracle parity tests/test_dzin_gpu.py and tests/test_elementwise_gpu.py hold): no tolerance anywhere in this file."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

NAN = float('nan')


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _full(n, v=NAN):
    return torch.full((int(n),), v, device='cuda')


# ---- 1. head: s mode equals da mode ---------------------------------------------------------------------------------------------

HEAD_PIXELS = [2 * 64 * 64, 1 * 40 * 72, 3 * 33 * 50]


def _head_case(L, C, pixels, seed):
    rs = np.random.RandomState(seed)
    c = dict(C=C, pixels=pixels, hb=L.dc_head_blocks(pixels))
    c['z'] = _dev(rs.standard_normal((pixels, C)).astype(np.float32))
    c['sc'] = _dev((rs.standard_normal(C) * 0.5 + 1.0).astype(np.float32))
    c['sh'] = _dev((rs.standard_normal(C) * 0.3).astype(np.float32))
    c['kh'] = _dev((rs.standard_normal((C, 2)) * 0.4).astype(np.float32))
    c['bh'] = _dev((rs.standard_normal(2) * 0.1).astype(np.float32))
    c['y'] = _dev((rs.random_sample(pixels) < 0.2).astype(np.uint8))
    c['mu'] = _dev((rs.standard_normal(C) * 0.2).astype(np.float32))
    c['istd'] = _dev((rs.random_sample(C) + 0.5).astype(np.float32))
    c['kd'] = c['kh'][:, 1] - c['kh'][:, 0]                        # fp32, one rounding: head_lane's kd
    return c


def _head_outputs(c):
    hb, C = c['hb'], c['C']
    # the partial rows are padded (C + 4 floats, C + 1 written): zeros, so that whole buffers compare
    return dict(p=_full(c['pixels']), part=_full(hb * 12), gpart=_full(hb * (C + 4), 0.0), bnp=_full(hb * C * 2), amx=_full(hb * C))


def _same(a, b, names):
    for n in names:
        assert not torch.isnan(a[n]).any(), n
        assert torch.equal(a[n], b[n]), n


@pytest.mark.parametrize('pixels', HEAD_PIXELS)
@pytest.mark.parametrize('C', [32, 16])
@pytest.mark.parametrize('kind', [0, 1])
def test_fused_head_s_mode_equals_da_mode(dclib, C, pixels, kind):
    L = dclib
    c = _head_case(L, C, pixels, 7 * C + kind + pixels % 97)
    old, new = _head_outputs(c), _head_outputs(c)
    da, s = _full(pixels * C), _full(pixels)
    untouched = _full(pixels * C)
    for fn, o, grad in ((L.dc_head_fwd_bwd, old, da), (L.dc_head_fwd_bwd_s, new, s)):
        fn(c['z'].data_ptr(), c['sc'].data_ptr(), c['sh'].data_ptr(), c['kh'].data_ptr(), c['bh'].data_ptr(), c['y'].data_ptr(),
           o['p'].data_ptr(), o['part'].data_ptr(), grad.data_ptr(), o['gpart'].data_ptr(), kind, c['mu'].data_ptr(),
           c['istd'].data_ptr(), o['bnp'].data_ptr(), o['amx'].data_ptr(), pixels, C, None)
    torch.cuda.synchronize()
    assert not torch.isnan(s).any() and not torch.isnan(da).any()
    assert torch.equal(da.view(pixels, C), s[:, None] * c['kd'][None, :])
    _same(old, new, ('p', 'part', 'gpart', 'bnp', 'amx'))
    assert torch.isnan(untouched).all()
    # a materialised input (in_scale NULL, no BatchNorm sums) through the same two entry points
    old, new = _head_outputs(c), _head_outputs(c)
    da, s = _full(pixels * C), _full(pixels)
    for fn, o, grad in ((L.dc_head_fwd_bwd, old, da), (L.dc_head_fwd_bwd_s, new, s)):
        fn(c['z'].data_ptr(), None, None, c['kh'].data_ptr(), c['bh'].data_ptr(), c['y'].data_ptr(), o['p'].data_ptr(),
           o['part'].data_ptr(), grad.data_ptr(), o['gpart'].data_ptr(), kind, None, None, None, None, pixels, C, None)
    torch.cuda.synchronize()
    assert torch.equal(da.view(pixels, C), s[:, None] * c['kd'][None, :])
    _same(old, new, ('p', 'part', 'gpart'))


@pytest.mark.parametrize('pixels', HEAD_PIXELS)
@pytest.mark.parametrize('C', [32, 16])
@pytest.mark.parametrize('kind', [0, 1, 2, 3])
def test_standalone_head_backward_s_mode_equals_da_mode(dclib, C, pixels, kind):
    L = dclib
    c = _head_case(L, C, pixels, 11 * C + kind + pixels % 89)
    hb = c['hb']
    p, part = _full(pixels), _full(hb * 12)
    sums = torch.zeros(12, dtype=torch.float64, device='cuda')
    L.dc_head_fwd_bnin(c['z'].data_ptr(), c['sc'].data_ptr(), c['sh'].data_ptr(), c['kh'].data_ptr(), c['bh'].data_ptr(),
                       c['y'].data_ptr(), p.data_ptr(), part.data_ptr(), pixels, C, None)
    L.dc_reduce_partials_f64(part.data_ptr(), hb, 12, sums.data_ptr(), None)
    old, new = _head_outputs(c), _head_outputs(c)
    da, s = _full(pixels * C), _full(pixels)
    untouched = _full(pixels * C)
    for fn, o, grad in ((L.dc_head_bwd_bnin_bnred, old, da), (L.dc_head_bwd_bnin_bnred_s, new, s)):
        fn(c['z'].data_ptr(), c['sc'].data_ptr(), c['sh'].data_ptr(), p.data_ptr(), c['y'].data_ptr(), c['kh'].data_ptr(),
           grad.data_ptr(), o['gpart'].data_ptr(), kind, sums.data_ptr(), c['mu'].data_ptr(), c['istd'].data_ptr(),
           o['bnp'].data_ptr(), o['amx'].data_ptr(), pixels, C, None)
    torch.cuda.synchronize()
    assert not torch.isnan(s).any() and not torch.isnan(da).any()
    assert torch.equal(da.view(pixels, C), s[:, None] * c['kd'][None, :])
    _same(old, new, ('gpart', 'bnp', 'amx'))
    assert torch.isnan(untouched).all()


# ---- dz-on-load table of a block (dc_bn_bwd_reduce -> dc_bn_bwd_finalize_dzin), inputs on the device -----------------------------

def _bn_of(z):
    """Batch statistics of a device tensor [.., C] + random affine -> (mean, invstd, gamma, beta) device fp32."""
    C = z.shape[-1]
    z64 = z.reshape(-1, C).double()
    mean = z64.mean(0).float()
    invstd = (1.0 / torch.sqrt(z64.var(0, unbiased=False) + 1e-3)).float()
    g = torch.Generator(device='cpu').manual_seed(C + z.numel() % 1000)
    gamma = (torch.randn(C, generator=g) * 0.7 + 1.0).cuda()
    beta = (torch.randn(C, generator=g) * 0.4).cuda()
    return mean.contiguous(), invstd.contiguous(), gamma, beta


def _dz_table(L, z, da, bn):
    C = z.shape[-1]
    M = z.numel() // C
    mean, invstd, gamma, beta = bn
    blocks = L.dc_bn_bwd_blocks(M, C)
    part, amx = _full(blocks * C * 2), _full(blocks * C)
    L.dc_bn_bwd_reduce(da.data_ptr(), C, z.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), None, 1.0, 0,
                       part.data_ptr(), amx.data_ptr(), M, C, None)
    dg, db, coef, dbias = _full(C), _full(C), _full(7 * C), _full(C)
    L.dc_bn_bwd_finalize_dzin(part.data_ptr(), amx.data_ptr(), blocks, C, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
                              beta.data_ptr(), float(M), dg.data_ptr(), db.data_ptr(), coef.data_ptr(), dbias.data_ptr(), None)
    torch.cuda.synchronize()
    return coef


# ---- 2. joint kernel: rank-one equals materialised -------------------------------------------------------------------------------

@pytest.mark.parametrize('N,H,W', [(2, 64, 64), (1, 40, 72), (3, 33, 50), (16, 32, 32)])
@pytest.mark.parametrize('bnin', [True, False])
def test_joint_rank_one_equals_materialised(dclib, N, H, W, bnin):
    """dc_conv3x3_bwd_joint_r1_f16x3 on (s, kh) against dc_conv3x3_bwd_joint_f16x3 fed da = s (x) kd: dx, dW and the fused sums of
    the layer in front, bit for bit; interior and ragged tiles, more tiles than workgroups and fewer; run-to-run equal."""
    L = dclib
    C = 32
    rows = L.dc_conv3x3_bwd_joint_blocks(N, H, W, C, C)
    assert rows > 0
    rs = np.random.RandomState(H * 7 + W + bnin)
    pixels = N * H * W
    s_np = (rs.standard_normal(pixels) * 3e-3).astype(np.float32)
    s_np[rs.random_sample(pixels) < 0.1] = 0.0                     # the loss' clip: exact zeros
    s = _dev(s_np)
    kh = _dev((rs.standard_normal((C, 2)) * 0.4).astype(np.float32))
    da = (s[:, None] * (kh[:, 1] - kh[:, 0])[None, :]).contiguous()
    z = _dev(rs.standard_normal((N, H, W, C)).astype(np.float32) * (rs.random_sample(C).astype(np.float32) + 0.5))
    x = _dev(rs.standard_normal((N, H, W, C)).astype(np.float32))
    coef = _dz_table(L, z, da, _bn_of(z))
    K = _dev((rs.standard_normal((3, 3, C, C)) * 0.05).astype(np.float32))
    wpd = torch.empty(L.dc_pack_weights_f16x3_floats(9, C, C), device='cuda')
    L.dc_pack_weights_f16x3(K.data_ptr(), wpd.data_ptr(), 9, C, C, C * C, 1, C, 1, None)
    ws = torch.empty(L.dc_conv3x3_bwd_joint_ws_floats(N, H, W, C, C), device='cuda')
    rmu, ris = _dev((rs.standard_normal(C) * 0.2).astype(np.float32)), _dev((rs.random_sample(C) + 0.5).astype(np.float32))
    rga, rbe = _dev((rs.standard_normal(C) * 0.5 + 1.0).astype(np.float32)), _dev((rs.standard_normal(C) * 0.3).astype(np.float32))
    xsc = (rga * ris).contiguous()
    xsh = (rbe - rmu * xsc).contiguous()

    def run(rank_one, sums=True):
        dx, dw = _full(pixels * C), _full(9 * C * C)
        part, amx = _full(rows * C * 2), _full(rows * C)
        red = (None,) * 7
        if sums:
            red = (x.data_ptr(), rmu.data_ptr(), ris.data_ptr(), rga.data_ptr(), rbe.data_ptr(), part.data_ptr(), amx.data_ptr())
        head = (x.data_ptr(), xsc.data_ptr() if bnin else None, xsh.data_ptr() if bnin else None, None)
        tail = (z.data_ptr(), coef.data_ptr(), wpd.data_ptr(), dx.data_ptr()) + red + (dw.data_ptr(), ws.data_ptr(), N, H, W, C, C, None)
        if rank_one:
            L.dc_conv3x3_bwd_joint_r1_f16x3(*(head + (s.data_ptr(), kh.data_ptr()) + tail))
        else:
            L.dc_conv3x3_bwd_joint_f16x3(*(head + (da.data_ptr(),) + tail))
        torch.cuda.synchronize()
        return dict(dx=dx, dw=dw, part=part, amx=amx)

    ref, got, again = run(False), run(True), run(True)
    _same(ref, got, ('dx', 'dw', 'part', 'amx'))
    _same(got, again, ('dx', 'dw', 'part', 'amx'))
    ref0, got0 = run(False, sums=False), run(True, sums=False)
    _same(ref0, got0, ('dx', 'dw'))
    assert torch.equal(got0['dx'], got['dx']) and torch.isnan(got0['part']).all() and torch.isnan(got0['amx']).all()


def test_joint_rank_one_serves_32_to_32_only(dclib):
    from deep_calcium_amd._lib import DcunetError
    L = dclib
    t = torch.zeros(4096, device='cuda')
    with pytest.raises(DcunetError, match=r'failed \(-3\)'):
        L.dc_conv3x3_bwd_joint_r1_f16x3(t.data_ptr(), None, None, None, t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(),
                                        t.data_ptr(), *((None,) * 7), t.data_ptr(), t.data_ptr(), 1, 32, 32, 64, 32, None)


# ---- 3. first layer's weight gradient: recomputed z equals stored z --------------------------------------------------------------

@pytest.mark.parametrize('N,H,W', [(2, 64, 64), (1, 40, 72), (3, 36, 52)])
@pytest.mark.parametrize('Cout', [32, 16])
def test_first_layer_wgrad_recomputed_z_equals_stored_z(dclib, N, H, W, Cout):
    L = dclib
    rs = np.random.RandomState(H + W + Cout)
    x = _dev((rs.standard_normal((N, H, W)) + 3.0).astype(np.float32))          # a DC offset of a few units
    w = _dev((rs.standard_normal((3, 3, 1, Cout)) * 0.3).astype(np.float32))
    bias = _dev((rs.standard_normal(Cout) * 0.5 + 0.25).astype(np.float32))
    z = _full(N * H * W * Cout).view(N, H, W, Cout)
    L.dc_conv3x3_c1_fwd(x.data_ptr(), w.data_ptr(), bias.data_ptr(), z.data_ptr(), Cout, None, None, None, 0, None, 0, N, H, W, Cout, None)
    torch.cuda.synchronize()
    assert not torch.isnan(z).any()
    da = _dev((rs.standard_normal((N, H, W, Cout)) * 3e-3).astype(np.float32))
    coef = _dz_table(L, z, da, _bn_of(z))
    ws = torch.empty(L.dc_conv3x3_wgrad_ws_floats(N, H, W, 1, Cout), device='cuda')
    dw_old, dw_new, dw_again = _full(9 * Cout), _full(9 * Cout), _full(9 * Cout)
    L.dc_conv3x3_wgrad_dzin_f16x3(x.data_ptr(), None, None, None, da.data_ptr(), z.data_ptr(), coef.data_ptr(), dw_old.data_ptr(),
                                  ws.data_ptr(), N, H, W, 1, Cout, None)
    for dw in (dw_new, dw_again):
        L.dc_conv3x3_c1_wgrad_dzin_zre(x.data_ptr(), w.data_ptr(), bias.data_ptr(), da.data_ptr(), coef.data_ptr(), dw.data_ptr(),
                                       ws.data_ptr(), N, H, W, Cout, None)
    torch.cuda.synchronize()
    assert not torch.isnan(dw_old).any() and dw_old.abs().max() > 0
    assert torch.equal(dw_old, dw_new) and torch.equal(dw_new, dw_again)


def test_first_layer_wgrad_recomputed_z_refuses_other_widths(dclib):
    from deep_calcium_amd._lib import DcunetError
    L = dclib
    N, H, W, Cout = 3, 33, 50, 32
    t = torch.zeros(N * H * W * Cout, device='cuda')
    with pytest.raises(DcunetError, match=r'failed \(-3\)'):
        L.dc_conv3x3_c1_wgrad_dzin_zre(t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(), t.data_ptr(),
                                       N, H, W, Cout, None)


# ---- 4. engine -------------------------------------------------------------------------------------------------------------------

HW, NFB, B = 256, 32, 17           # N*H*W just above 2^20: the dz-on-load branch; a step takes a few ms
NEW = ('dc_head_fwd_bwd_s', 'dc_conv3x3_bwd_joint_r1_f16x3', 'dc_conv3x3_c1_wgrad_dzin_zre')


class _Counting(object):
    """Proxy in front of the engine's library object: counts the dc_* calls by name (and the joint launches by channel pair)."""
    def __init__(self, lib):
        self._lib, self.calls, self.first_layer_old = lib, {}, 0

    def __getattr__(self, name):
        attr = getattr(self._lib, name)
        if not name.startswith('dc_') or not callable(attr):
            return attr

        def counted(*a):
            self.calls[name] = self.calls.get(name, 0) + 1
            if name == 'dc_conv3x3_wgrad_dzin_f16x3' and a[12] == 1:          # (.., N, H, W, Cin, Cout, stream)
                self.first_layer_old += 1
            return attr(*a)
        return counted


@pytest.fixture(scope='module')
def engine_batches():
    rs = np.random.RandomState(31)
    return [(_dev(rs.standard_normal((B, HW, HW)).astype(np.float32)), _dev((rs.random_sample((B, HW, HW)) < 0.15).astype(np.uint8)))
            for _ in range(2)]


def _train(batches, on, tapes, steps, flips=(), count=False):
    """`steps` seeded train steps; flips: steps before which both attributes are inverted.  -> (metrics, gflat, pflat[, proxy])"""
    from deep_calcium_amd.model import Model, Adam
    m = Model((HW, HW), NFB)
    m.compile(Adam(0.002), 'binary_crossentropy')
    eng = m.engine
    eng.use_tapes = tapes
    eng.head_rank1 = eng.c1_z_on_load = on
    proxy = None
    if count:
        proxy = eng.L = _Counting(eng.L)
    hist = []
    for step in range(steps):
        if step in flips:
            eng.head_rank1 = eng.c1_z_on_load = not eng.head_rank1
        hist.append(m.train_on_device_batch(*batches[step % 2]))
    torch.cuda.synchronize()
    out = (hist, eng.gflat.clone(), eng.pflat.clone())
    if tapes and not flips:
        assert eng.tape_replays > 0
    return out + ((proxy,) if count else ())


def _equal_runs(a, b):
    assert a[0] == b[0]                                  # the returned metric lists of every step
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])


@pytest.fixture(scope='module')
def reference_run(engine_batches):
    """Four launch-by-launch steps with both attributes off (the existing entry points), counted: computed once, shared."""
    return _train(engine_batches, False, False, 4, count=True)


def test_engine_untaped_calls_the_new_entry_points_and_computes_the_same_step(engine_batches, reference_run):
    on = _train(engine_batches, True, False, 4, count=True)
    _equal_runs(reference_run, on)
    was, now = reference_run[3], on[3]
    assert all(was.calls.get(name, 0) == 0 for name in NEW)
    assert was.calls.get('dc_head_fwd_bwd', 0) == 4 and was.first_layer_old == 4
    for name in NEW:
        assert now.calls.get(name, 0) == 4, (name, now.calls.get(name))
    assert now.calls.get('dc_head_fwd_bwd', 0) == 0 and now.first_layer_old == 0
    # the existing joint entry point has lost exactly block d0b's launch of every step
    assert now.calls.get('dc_conv3x3_bwd_joint_f16x3', 0) == was.calls['dc_conv3x3_bwd_joint_f16x3'] - 4 > 0


@pytest.mark.parametrize('on', [True, False])
def test_engine_taped_equals_launch_by_launch(engine_batches, reference_run, on):
    _equal_runs(reference_run, _train(engine_batches, on, True, 4))          # steps 3 and 4 are replays


def test_engine_flipping_the_attributes_drops_the_tapes(engine_batches, reference_run):
    _equal_runs(reference_run, _train(engine_batches, True, True, 4, flips=(3,)))
    _equal_runs(reference_run, _train(engine_batches, False, False, 4, flips=(1, 2)))


def test_engine_dice_loss_takes_the_standalone_head_in_s_mode(engine_batches):
    """Loss kinds 2 / 3 run the head's backward on its own (dc_head_bwd_bnin_bnred_s)."""
    from deep_calcium_amd.model import Model, Adam
    out = []
    for on in (False, True):
        m = Model((HW, HW), NFB)
        m.compile(Adam(0.002), 'dice_loss')
        eng = m.engine
        eng.use_tapes = False
        eng.head_rank1 = eng.c1_z_on_load = on
        proxy = eng.L = _Counting(eng.L)
        hist = [m.train_on_device_batch(*engine_batches[0])]
        torch.cuda.synchronize()
        out.append((hist, eng.gflat.clone(), eng.pflat.clone()))
        assert proxy.calls.get('dc_head_bwd_bnin_bnred_s', 0) == (1 if on else 0)
        assert proxy.calls.get('dc_head_bwd_bnin_bnred', 0) == (0 if on else 1)
    _equal_runs(*out)
