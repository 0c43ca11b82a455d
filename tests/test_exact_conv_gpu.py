"""Every matrix kernel on exact-lattice data (tests/_lattice.py): EQUALITY with the one exactly known
result per element, through the C ABI.  The float64 expected values come from oracle/unet_numpy.py by linearity (the split-fp16
kernels drop lo*lo by definition: oracle(a, b) - oracle(a_lo, b_lo)); tests/test_lattice.py proves on the CPU, for every case
here (the z-rebuilt, statistics and guard cases included), the conditions under which any order of fp32 summation gives these bits.  Outputs start as NaN between NaN guard
elements; strided destinations keep their gap columns untouched."""
import os

import numpy as np
import pytest

import _lattice as lt
import _tileplan as tp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

_KEEP = []
GUARD = 64


@pytest.fixture(autouse=True)
def _keep_alive():
    """device temporaries must outlive the asynchronous launches that read them (raw pointers cross the C ABI)"""
    yield
    torch.cuda.synchronize()
    del _KEEP[:]


def _fused_paths_enabled(*knobs):
    return all(os.environ.get(k, '1') != '0' for k in ('DC_IGEMM_PP',) + knobs)


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _KEEP.append(t)
    return t


class Out:
    """NaN-filled output with GUARD NaN elements on both sides; .np() asserts the guards are still NaN."""

    def __init__(self, *shape, dtype=torch.float32):
        n = int(np.prod(shape))
        self.flat = torch.full((n + 2 * GUARD,), float('nan'), device='cuda', dtype=dtype)
        self.view = self.flat[GUARD:GUARD + n].view(*shape)
        _KEEP.append(self.flat)

    def ptr(self, offset_elems=0):
        return self.view.data_ptr() + offset_elems * self.flat.element_size()

    def np(self):
        torch.cuda.synchronize()
        f = self.flat.cpu().numpy()
        assert np.isnan(f[:GUARD]).all() and np.isnan(f[-GUARD:]).all(), 'guard elements overwritten'
        return f[GUARD:-GUARD].reshape(tuple(self.view.shape))


def same(got, want, what=''):
    """np.array_equal with the first differing element in the message"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(~(got == want))
        i = tuple(bad[0])
        raise AssertionError('%s: %d of %d elements differ; first at %s: got %r, expected %r' % (what, len(bad), got.size, i, got[i], want[i]))


def strided(view_np, off, C, what):
    """[..., ld] buffer: columns [off, off + C) are the output, every other column is still NaN"""
    gap = np.ones(view_np.shape[-1], bool)
    gap[off:off + C] = False
    assert np.isnan(view_np[..., gap]).all(), '%s: gap columns of the strided destination written' % what
    return view_np[..., off:off + C]


def pack16(L, K, form, Ci, Co):
    """dc_pack_weights_f16x3 in one of the four forms of include/dcunet.h"""
    taps, Kd, Nc, st, sk, sn, flip = {'c3f': (9, Ci, Co, Ci * Co, Co, 1, 0), 'c3d': (9, Co, Ci, Ci * Co, 1, Co, 1),
                                      'ctf': (1, Ci, 4 * Co, 0, 1, Ci, 0), 'ctd': (4, Co, Ci, Co * Ci, Ci, 1, 0)}[form]
    wp = torch.empty(L.dc_pack_weights_f16x3_floats(taps, Kd, Nc), device='cuda')
    L.dc_pack_weights_f16x3(dev(K).data_ptr(), wp.data_ptr(), taps, Kd, Nc, st, sk, sn, flip, None)
    _KEEP.append(wp)
    return wp, (taps, Kd, Nc, st, sk, sn, flip)


def pack32(L, K, form, Ci, Co):
    taps, Kd, Nc, st, sk, sn, flip = {'c3f': (9, Ci, Co, Ci * Co, Co, 1, 0), 'c3d': (9, Co, Ci, Ci * Co, 1, Co, 1),
                                      'ctf': (1, Ci, 4 * Co, 0, 1, Ci, 0), 'ctd': (4, Co, Ci, Co * Ci, Ci, 1, 0),
                                      '1df': (5, Ci, Co, Ci * Co, Co, 1, 0)}[form]
    wp = torch.empty(taps * Kd * Nc, device='cuda')
    L.dc_pack_weights(dev(K).data_ptr(), wp.data_ptr(), taps, Kd, Nc, st, sk, sn, flip, None)
    _KEEP.append(wp)
    return wp


def dz_scalar(L, c):
    """the dz scale as a device scalar from the library's own kernel; equals the emulated power of two"""
    scl = torch.full((4,), float('nan'), device='cuda')
    L.dc_pow2_scale_from_absmax(dev(np.array([np.abs(c.dz).max()], np.float32)).data_ptr(), 1, 1024.0, scl.data_ptr(), None)
    torch.cuda.synchronize()
    _KEEP.append(scl)
    assert float(scl[0].item()) == c.s_dz
    return scl


def dz_blockmax(c):
    """per-block maxima as dc_bn_bwd_apply leaves them: the true maximum in one of 37 entries"""
    part = np.full(37, np.abs(c.dz).max() * 0.3, np.float32)
    part[11] = np.abs(c.dz).max()
    return dev(part)


def ids(v):
    return '-'.join(str(a) for a in v) if isinstance(v, tuple) else str(v)


# ------------------------------------------------------------------------------------------------------------ the premise
def test_premise_fp16_mfma_accumulates_exact_partial_sums_exactly(dclib):
    """FIRST: one plain dc_conv3x3_fwd_f16x3 on a single tile and a single K-chunk.  Nothing documents that the fp16 MFMA
    adds exactly representable partial sums exactly (the fp32-input one is a bitwise fmaf chain); every two-digit case below
    rests on it."""
    L = dclib
    N, H, W, Ci, Co = lt.PREMISE
    c = lt.conv_case('c3', *lt.PREMISE)
    wp, _ = pack16(L, c.K, 'c3f', Ci, Co)
    z = Out(N, H, W, Co)
    L.dc_conv3x3_fwd_f16x3(dev(c.x).data_ptr(), wp.data_ptr(), None, z.ptr(), Co, None, 0, None, None, 0, None, 0, None, 0, None,
                           N, H, W, Ci, Co, None)
    same(z.np(), c.z - lt.f64(c.bias), 'premise z')


# ---------------------------------------------------------------------------------------------------------- fp32-MFMA path
@pytest.mark.parametrize('case', lt.INT_F32, ids=ids)
def test_fp32_mfma_contractions_on_integers(dclib, case):
    """dc_conv3x3_{fwd,dgrad,wgrad} / dc_convT2x2_{fwd,dgrad,wgrad}: fp32 products of integers are exact (g = 1)."""
    L = dclib
    kind, N, H, W, Ci, Co = case
    c = lt.conv_case(kind, N, H, W, Ci, Co, False, 1.0)
    sc, sh, y = lt.epilogue(c)
    xd, dzd, bd = dev(c.x), dev(c.dz), dev(c.bias)
    if kind == 'c3':
        Ho, Wo = H, W
        fwd, dgrad, wgrad, wsf = L.dc_conv3x3_fwd, L.dc_conv3x3_dgrad, L.dc_conv3x3_wgrad, L.dc_conv3x3_wgrad_ws_floats
        wp, wpd, dw = pack32(L, c.K, 'c3f', Ci, Co), pack32(L, c.K, 'c3d', Ci, Co), Out(3, 3, Ci, Co)
    else:
        Ho, Wo = 2 * H, 2 * W
        fwd, dgrad, wgrad, wsf = L.dc_convT2x2_fwd, L.dc_convT2x2_dgrad, L.dc_convT2x2_wgrad, L.dc_convT2x2_wgrad_ws_floats
        wp, wpd, dw = pack32(L, c.K, 'ctf', Ci, Co), pack32(L, c.K, 'ctd', Ci, Co), Out(2, 2, Co, Ci)
    z, cat, dx = Out(N, Ho, Wo, Co), Out(N, Ho, Wo, 2 * Co + 4), Out(N, H, W, Ci)
    fwd(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), z.ptr(), Co, None, None, None, 0, N, H, W, Ci, Co, None)
    fwd(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), cat.ptr(Co), 2 * Co + 4, None, dev(sc).data_ptr(), dev(sh).data_ptr(), 1,
        N, H, W, Ci, Co, None)
    dgrad(dzd.data_ptr(), wpd.data_ptr(), dx.ptr(), N, H, W, Ci, Co, None)
    ws = torch.empty(max(wsf(N, H, W, Ci, Co), 4), device='cuda')
    wgrad(xd.data_ptr(), dzd.data_ptr(), dw.ptr(), ws.data_ptr(), N, H, W, Ci, Co, None)
    same(z.np(), c.z, 'z')
    same(strided(cat.np(), Co, Co, 'epilogue'), y, 'fused epilogue')
    same(dx.np(), c.dx, 'dx')
    same(dw.np(), c.dK, 'dW')


@pytest.mark.parametrize('shape', lt.C1, ids=ids)
def test_first_layer_forward_and_weight_gradient_on_integers(dclib, shape):
    """dc_conv3x3_c1_fwd (z, max |z| per channel) and the Cin == 1 route of dc_conv3x3_wgrad."""
    L = dclib
    N, H, W, Co = shape
    c = lt.c1_case(*shape)
    z, amx, dw = Out(N, H, W, Co), torch.zeros(Co, device='cuda'), Out(3, 3, 1, Co)
    xd = dev(c.x.reshape(N, H, W))
    L.dc_conv3x3_c1_fwd(xd.data_ptr(), dev(c.K).data_ptr(), dev(c.bias).data_ptr(), z.ptr(), Co, None, None, None, 0,
                        amx.data_ptr(), 0, N, H, W, Co, None)
    ws = torch.empty(L.dc_conv3x3_wgrad_ws_floats(N, H, W, 1, Co), device='cuda')
    L.dc_conv3x3_wgrad(xd.data_ptr(), dev(c.dz).data_ptr(), dw.ptr(), ws.data_ptr(), N, H, W, 1, Co, None)
    same(z.np(), c.z, 'z')
    same(amx.cpu().numpy(), np.abs(c.z).max((0, 1, 2)), 'max |z|')
    same(dw.np(), c.dK, 'dW')


@pytest.mark.parametrize('shape', lt.CONV1D + lt.CONV1D_C1, ids=ids)
def test_conv1d_forward_and_weight_gradient_on_integers(dclib, shape):
    """dc_conv1d_k5_fwd / _c1_fwd into a strided destination, dc_conv1d_k5_wgrad / _c1_wgrad."""
    L = dclib
    N, T, Ci, Co = shape
    c = lt.conv1d_case(*shape)
    ld = Co + 8
    y, dw = Out(N, T, ld), Out(5, Ci, Co)
    scd, shd, dzd = dev(c.scale), dev(c.shift), dev(c.dz)
    if Ci == 1:
        xd = dev(c.x.reshape(N, T))
        L.dc_conv1d_k5_c1_fwd(xd.data_ptr(), dev(c.K).data_ptr(), scd.data_ptr(), shd.data_ptr(), 1, y.ptr(4), ld, N, T, Co, None)
        ws = torch.empty(max(L.dc_conv1d_k5_c1_wgrad_ws_floats(N, T, Co), 4), device='cuda')
        L.dc_conv1d_k5_c1_wgrad(xd.data_ptr(), dzd.data_ptr(), dw.ptr(), ws.data_ptr(), N, T, Co, None)
    else:
        xd = dev(c.x)
        L.dc_conv1d_k5_fwd(xd.data_ptr(), pack32(L, c.K, '1df', Ci, Co).data_ptr(), scd.data_ptr(), shd.data_ptr(), 1, y.ptr(4), ld,
                           N, T, Ci, Co, None)
        ws = torch.empty(max(L.dc_conv1d_k5_wgrad_ws_floats(N, T, Ci, Co), 4), device='cuda')
        L.dc_conv1d_k5_wgrad(xd.data_ptr(), dzd.data_ptr(), dw.ptr(), ws.data_ptr(), N, T, Ci, Co, None)
    same(strided(y.np(), 4, Co, 'conv1d'), c.y, 'y')
    same(dw.np(), c.dK, 'dW')


# -------------------------------------------------------------------------------------------------------- split-fp16 path
@pytest.mark.parametrize('case', [('c3',) + lt.CONV3[1], ('c3',) + lt.CONV3[3], ('ct',) + lt.CONVT[0]], ids=ids)
def test_pack_weights_f16x3_planes_and_trailer(dclib, case):
    """hi plane, lo plane and trailer of the forward and the data-gradient image against the emulated split."""
    L = dclib
    kind, N, H, W, Ci, Co = case
    c = lt.conv_case(*case)
    for form in (('c3f', 'c3d') if kind == 'c3' else ('ctf', 'ctd')):
        wp, args = pack16(L, c.K, form, Ci, Co)
        torch.cuda.synchronize()
        raw = wp.cpu().numpy()
        img, ws, amax = lt.pack_image(c.K, *args)
        assert np.array_equal(raw[:-4].view(np.uint16), img.view(np.uint16)), form
        assert raw[-4] == ws == c.s_k and raw[-3] == amax


# the shapes that are here for their split over K; the two deep ones at N = 1, the smallest batch there is
SPLITK = {(1, 8, 8, 512, 512), (1, 16, 16, 256, 256), (3, 12, 12, 200, 96)}


@pytest.mark.parametrize('shape', lt.CONV3, ids=ids)
def test_conv3x3_f16x3_two_digit(dclib, shape):
    """dc_conv3x3_fwd_f16x3 (plain with bias; fused epilogue into a strided destination with out_absmax; split over K and not),
    dc_conv3x3_dgrad_f16x3 (scale as a device scalar and as per-block maxima), dc_conv3x3_wgrad_f16x3."""
    L = dclib
    N, H, W, Ci, Co = shape
    c = lt.conv_case('c3', *shape)
    sc, sh, y = lt.epilogue(c)
    xd, dzd, bd = dev(c.x), dev(c.dz), dev(c.bias)
    wp, _ = pack16(L, c.K, 'c3f', Ci, Co)
    wpd, _ = pack16(L, c.K, 'c3d', Ci, Co)
    skf, skd = L.dc_conv3x3_splitk_ws_floats(N, H, W, Ci, Co, 0), L.dc_conv3x3_splitk_ws_floats(N, H, W, Ci, Co, 1)
    if shape in SPLITK:
        assert skf > 0 and skd > 0, 'this shape is here for its split over K'
    skws = torch.full((max(skf, skd, 4),), float('nan'), device='cuda')
    z, z1, cat = Out(N, H, W, Co), Out(N, H, W, Co), Out(N, H, W, Co + 12)
    L.dc_conv3x3_fwd_f16x3(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), z.ptr(), Co, None, 0, None, None, 0, None, 0, None, 0,
                           skws.data_ptr(), N, H, W, Ci, Co, None)
    same(z.np(), c.z, 'z')
    # no workspace: ONE un-split launch -- another order of summation, the same bits on this data
    L.dc_conv3x3_fwd_f16x3(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), z1.ptr(), Co, None, 0, None, None, 0, None, 0, None, 0,
                           None, N, H, W, Ci, Co, None)
    same(z1.np(), c.z, 'z, not split')
    amx = torch.zeros(Co, device='cuda')
    L.dc_conv3x3_fwd_f16x3(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), cat.ptr(8), Co + 12, None, 0, dev(sc).data_ptr(),
                           dev(sh).data_ptr(), 1, None, 0, amx.data_ptr(), 0, skws.data_ptr(), N, H, W, Ci, Co, None)
    same(strided(cat.np(), 8, Co, 'epilogue'), y, 'fused epilogue')
    same(amx.cpu().numpy(), y.max((0, 1, 2)), 'measured max |output|')
    dx, dxa, dw = Out(N, H, W, Ci), Out(N, H, W, Ci), Out(3, 3, Ci, Co)
    scl = dz_scalar(L, c)
    L.dc_conv3x3_dgrad_f16x3(dzd.data_ptr(), wpd.data_ptr(), dx.ptr(), scl.data_ptr(), None, 0, skws.data_ptr(), N, H, W, Ci, Co, None)
    same(dx.np(), c.dx, 'dx, scalar scale')
    L.dc_conv3x3_dgrad_f16x3(dzd.data_ptr(), wpd.data_ptr(), dxa.ptr(), None, dz_blockmax(c).data_ptr(), 37, skws.data_ptr(),
                             N, H, W, Ci, Co, None)
    same(dxa.np(), c.dx, 'dx, per-block maxima')
    ws = torch.empty(L.dc_conv3x3_wgrad_ws_floats(N, H, W, Ci, Co), device='cuda')
    L.dc_conv3x3_wgrad_f16x3(xd.data_ptr(), dzd.data_ptr(), dw.ptr(), ws.data_ptr(), scl.data_ptr(), None, N, H, W, Ci, Co, None)
    same(dw.np(), c.dK, 'dW')


@pytest.mark.parametrize('shape', lt.CONVT, ids=ids)
def test_convT2x2_f16x3_two_digit(dclib, shape):
    """The three dc_convT2x2_*_f16x3: forward plain and with the fused epilogue into a strided destination (max |output| per
    channel measured), data gradient under both scale forms, weight gradient."""
    L = dclib
    N, H, W, Ci, Co = shape
    c = lt.conv_case('ct', *shape)
    sc, sh, y = lt.epilogue(c)
    xd, dzd, bd = dev(c.x), dev(c.dz), dev(c.bias)
    wp, _ = pack16(L, c.K, 'ctf', Ci, Co)
    wpd, _ = pack16(L, c.K, 'ctd', Ci, Co)
    z, cat = Out(N, 2 * H, 2 * W, Co), Out(N, 2 * H, 2 * W, 2 * Co)
    amx = torch.zeros(Co, device='cuda')
    L.dc_convT2x2_fwd_f16x3(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), z.ptr(), Co, None, None, None, 0, None, 0, None, 0,
                            N, H, W, Ci, Co, None)
    L.dc_convT2x2_fwd_f16x3(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), cat.ptr(Co), 2 * Co, None, dev(sc).data_ptr(),
                            dev(sh).data_ptr(), 1, None, 0, amx.data_ptr(), 0, N, H, W, Ci, Co, None)
    same(z.np(), c.z, 'z')
    same(strided(cat.np(), Co, Co, 'epilogue'), y, 'fused epilogue')
    same(amx.cpu().numpy(), y.max((0, 1, 2)), 'measured max |output|')
    skn = L.dc_convT2x2_dgrad_splitk_ws_floats(N, H, W, Ci, Co)
    skws = torch.full((max(skn, 4),), float('nan'), device='cuda')
    dx, dxa, dw = Out(N, H, W, Ci), Out(N, H, W, Ci), Out(2, 2, Co, Ci)
    scl = dz_scalar(L, c)
    L.dc_convT2x2_dgrad_f16x3(dzd.data_ptr(), wpd.data_ptr(), dx.ptr(), scl.data_ptr(), None, 0, skws.data_ptr(), N, H, W, Ci, Co, None)
    L.dc_convT2x2_dgrad_f16x3(dzd.data_ptr(), wpd.data_ptr(), dxa.ptr(), None, dz_blockmax(c).data_ptr(), 37, None, N, H, W, Ci, Co, None)
    ws = torch.empty(L.dc_convT2x2_wgrad_ws_floats(N, H, W, Ci, Co), device='cuda')
    L.dc_convT2x2_wgrad_f16x3(xd.data_ptr(), dzd.data_ptr(), dw.ptr(), ws.data_ptr(), scl.data_ptr(), None, N, H, W, Ci, Co, None)
    same(dx.np(), c.dx, 'dx, scalar scale')
    same(dxa.np(), c.dx, 'dx, per-block maxima, not split')
    same(dw.np(), c.dK, 'dW')


@pytest.mark.parametrize('case', lt.STATS, ids=ids)
def test_f16x3_forward_stats_rows_on_small_integers(dclib, case):
    """The float64 BatchNorm rows of dc_conv3x3_fwd_f16x3, dc_convT2x2_fwd_f16x3 and their _bnin forms: integer z small enough
    that the fp32 shifted sums and Chan merges behind them are exact (lt.stats_case states the condition: 8 x 8 tiles inside
    the image, asserted here through the row count), so the rows sum to the integer sums of z and z^2."""
    L = dclib
    kind, N, H, W, Ci, Co, tile_pixels, bnin = case
    c = lt.stats_case(*case)
    if kind == 'c3':
        tiles, cols, Ho, Wo = L.dc_conv3x3_tiles(N, H, W, Co), Co, H, W
    else:
        tiles, cols, Ho, Wo = L.dc_convT2x2_f16x3_tiles(N, H, W, Co), 4 * Co, 2 * H, 2 * W
    assert tiles * tile_pixels == N * H * W, 'the rows are not one per full 8 x 8 tile'
    wp, _ = pack16(L, c.K, 'c3f' if kind == 'c3' else 'ctf', Ci, Co)
    z, st = Out(N, Ho, Wo, Co), Out(tiles * cols * 2, dtype=torch.float64)
    if bnin:
        on_load = (dev(c.z_in).data_ptr(), dev(c.in_scale).data_ptr(), dev(c.in_shift).data_ptr(), dev(c.abound).data_ptr())
        if kind == 'c3':
            L.dc_conv3x3_fwd_bnin_f16x3(*on_load, wp.data_ptr(), None, z.ptr(), Co, st.ptr(), 0, None, None, 0, None, N, H, W, Ci, Co, None)
        else:
            L.dc_convT2x2_fwd_bnin_f16x3(*on_load, wp.data_ptr(), None, z.ptr(), Co, st.ptr(), None, None, 0, N, H, W, Ci, Co, None)
    elif kind == 'c3':
        L.dc_conv3x3_fwd_f16x3(dev(c.x).data_ptr(), wp.data_ptr(), None, z.ptr(), Co, st.ptr(), 0, None, None, 0, None, 0, None, 0, None,
                               N, H, W, Ci, Co, None)
    else:
        L.dc_convT2x2_fwd_f16x3(dev(c.x).data_ptr(), wp.data_ptr(), None, z.ptr(), Co, st.ptr(), None, None, 0, None, 0, None, 0,
                                N, H, W, Ci, Co, None)
    same(z.np(), c.z, 'z')
    rows = st.np().reshape(tiles, cols // Co, Co, 2).sum((0, 1))          # conv-transpose: the four taps are column groups
    same(rows, c.sums, 'sum z, sum z^2 over the rows')


def test_first_layer_forward_stats_rows_on_integers(dclib):
    """dc_conv3x3_c1_fwd's float64 rows at Cout = 512: two pixel lanes per block, one 4-pixel group each (lt.c1_stats_case)."""
    L = dclib
    N, H, W, Co = lt.C1_STATS
    c = lt.c1_stats_case(*lt.C1_STATS)
    tiles = L.dc_conv3x3_c1_tiles(N, H, W, Co)
    assert tiles == N * H * W // 2, 'not two pixel lanes per block'
    z, st = Out(N, H, W, Co), Out(tiles, Co, 2, dtype=torch.float64)
    L.dc_conv3x3_c1_fwd(dev(c.x.reshape(N, H, W)).data_ptr(), dev(c.K).data_ptr(), dev(c.bias).data_ptr(), z.ptr(), Co, st.ptr(),
                        None, None, 0, None, 0, N, H, W, Co, None)
    same(z.np(), c.z, 'z')
    same(st.np().sum(0), c.sums, 'sum z, sum z^2 over the rows')


@pytest.mark.parametrize('case', lt.GUARDED, ids=ids)
def test_plain_f16x3_kernels_under_the_activation_guard(dclib, case):
    """in_abound of the two plain forwards and x_abound of the two plain weight gradients: x is split under 2^13."""
    L = dclib
    kind, N, H, W, Ci, Co = case
    c = lt.conv_case(kind, N, H, W, Ci, Co, True, lt.GRAD, True)
    assert c.s_x == 2.0 ** 13
    xd, abd, scl = dev(c.x), dev(c.abound), dz_scalar(L, c)
    wp, _ = pack16(L, c.K, 'c3f' if kind == 'c3' else 'ctf', Ci, Co)
    if kind == 'c3':
        z, dw = Out(N, H, W, Co), Out(3, 3, Ci, Co)
        L.dc_conv3x3_fwd_f16x3(xd.data_ptr(), wp.data_ptr(), dev(c.bias).data_ptr(), z.ptr(), Co, None, 0, None, None, 0, abd.data_ptr(), 0,
                               None, 0, None, N, H, W, Ci, Co, None)
        ws = torch.empty(L.dc_conv3x3_wgrad_ws_floats(N, H, W, Ci, Co), device='cuda')
        L.dc_conv3x3_wgrad_f16x3(xd.data_ptr(), dev(c.dz).data_ptr(), dw.ptr(), ws.data_ptr(), scl.data_ptr(), abd.data_ptr(),
                                 N, H, W, Ci, Co, None)
    else:
        z, dw = Out(N, 2 * H, 2 * W, Co), Out(2, 2, Co, Ci)
        L.dc_convT2x2_fwd_f16x3(xd.data_ptr(), wp.data_ptr(), dev(c.bias).data_ptr(), z.ptr(), Co, None, None, None, 0, abd.data_ptr(), 0,
                                None, 0, N, H, W, Ci, Co, None)
        ws = torch.empty(L.dc_convT2x2_wgrad_ws_floats(N, H, W, Ci, Co), device='cuda')
        L.dc_convT2x2_wgrad_f16x3(xd.data_ptr(), dev(c.dz).data_ptr(), dw.ptr(), ws.data_ptr(), scl.data_ptr(), abd.data_ptr(),
                                  N, H, W, Ci, Co, None)
    same(z.np(), c.z, 'z')
    same(dw.np(), c.dK, 'dW')


@pytest.mark.parametrize('case', lt.BNIN, ids=ids)
def test_bn_relu_on_load_two_digit(dclib, case):
    """The four _bnin_f16x3 entry points: relu(fmaf(z_in, in_scale, in_shift)) formed while staging, under the guard scale of
    in_abound; positive shifts must not leak into the zero padding."""
    L = dclib
    kind, N, H, W, Ci, Co = case
    c = lt.bnin_case(*case)
    zin, scd, shd, abd, dzd = dev(c.z_in), dev(c.in_scale), dev(c.in_shift), dev(c.abound), dev(c.dz)
    scl = dz_scalar(L, c)
    if kind == 'c3':
        wp, _ = pack16(L, c.K, 'c3f', Ci, Co)
        z, dw = Out(N, H, W, Co + 4), Out(3, 3, Ci, Co)
        skf = L.dc_conv3x3_splitk_ws_floats(N, H, W, Ci, Co, 0)
        skws = torch.full((max(skf, 4),), float('nan'), device='cuda')
        L.dc_conv3x3_fwd_bnin_f16x3(zin.data_ptr(), scd.data_ptr(), shd.data_ptr(), abd.data_ptr(), wp.data_ptr(), None, z.ptr(4), Co + 4,
                                    None, 0, None, None, 0, skws.data_ptr(), N, H, W, Ci, Co, None)
        ws = torch.empty(L.dc_conv3x3_wgrad_ws_floats(N, H, W, Ci, Co), device='cuda')
        L.dc_conv3x3_wgrad_bnin_f16x3(zin.data_ptr(), scd.data_ptr(), shd.data_ptr(), abd.data_ptr(), dzd.data_ptr(), dw.ptr(),
                                      ws.data_ptr(), scl.data_ptr(), N, H, W, Ci, Co, None)
    else:
        wp, _ = pack16(L, c.K, 'ctf', Ci, Co)
        z, dw = Out(N, 2 * H, 2 * W, Co + 4), Out(2, 2, Co, Ci)
        L.dc_convT2x2_fwd_bnin_f16x3(zin.data_ptr(), scd.data_ptr(), shd.data_ptr(), abd.data_ptr(), wp.data_ptr(), None, z.ptr(4), Co + 4,
                                     None, None, None, 0, N, H, W, Ci, Co, None)
        ws = torch.empty(L.dc_convT2x2_wgrad_ws_floats(N, H, W, Ci, Co), device='cuda')
        L.dc_convT2x2_wgrad_bnin_f16x3(zin.data_ptr(), scd.data_ptr(), shd.data_ptr(), abd.data_ptr(), dzd.data_ptr(), dw.ptr(),
                                       ws.data_ptr(), scl.data_ptr(), N, H, W, Ci, Co, None)
    same(strided(z.np(), 4, Co, 'bnin forward'), c.z, 'z')
    same(dw.np(), c.dK, 'dW')


@pytest.mark.parametrize('shape', lt.POOL, ids=ids)
def test_conv3x3_fwd_pool_f16x3_two_digit(dclib, shape):
    """Inference forward that also writes the 2 x 2 max pool of its (strided) output."""
    L = dclib
    N, H, W, Ci, Co = shape
    if L.dc_conv3x3_fwd_pool_blocks(N, H, W, Ci, Co) == 0:
        assert not _fused_paths_enabled()
        pytest.skip('pooled forward switched off by an A/B knob')
    c = lt.conv_case('c3', *shape)
    sc, sh, y = lt.epilogue(c)
    wp, _ = pack16(L, c.K, 'c3f', Ci, Co)
    cat, pool = Out(N, H, W, 2 * Co), Out(N, H // 2, W // 2, Co)
    flag = torch.zeros(4, device='cuda')
    L.dc_conv3x3_fwd_pool_f16x3(dev(c.x).data_ptr(), wp.data_ptr(), dev(c.bias).data_ptr(), cat.ptr(Co), 2 * Co, dev(sc).data_ptr(),
                                dev(sh).data_ptr(), 1, flag.data_ptr(), pool.ptr(), N, H, W, Ci, Co, None)
    same(strided(cat.np(), Co, Co, 'pooled forward'), y, 'y')
    same(pool.np(), lt.maxpool(y), 'pool')
    assert float(flag[0].item()) == 0.0


@pytest.mark.parametrize('case', lt.BNRED, ids=ids)
def test_dgrad_bnred_f16x3(dclib, case):
    """dc_conv3x3_dgrad_bnred_f16x3 / dc_convT2x2_dgrad_bnred_f16x3: dx on two-digit data, and on integers dx together with the
    pass-1 sums (sum dy, sum dy xhat) and max |dy| of the layer in front -- EQUAL to the integer sums."""
    L = dclib
    kind, N, H, W, Ci, Co = case
    blocks = (L.dc_conv3x3_dgrad_bnred_blocks if kind == 'c3' else L.dc_convT2x2_dgrad_bnred_blocks)(N, H, W, Ci, Co)
    if blocks == 0:
        assert not _fused_paths_enabled()
        pytest.skip('fused sums switched off by an A/B knob')
    entry = L.dc_conv3x3_dgrad_bnred_f16x3 if kind == 'c3' else L.dc_convT2x2_dgrad_bnred_f16x3
    r = lt.bnred_case(*case)
    bn = r.bn
    zf, mu, isd, ga, be = dev(r.zf), dev(bn.mean), dev(bn.invstd), dev(bn.gamma), dev(bn.beta)
    for c, sums, blockmax in ((lt.conv_case(*case), False, False), (r.conv, True, False), (r.conv, True, True)):
        wpd, _ = pack16(L, c.K, 'c3d' if kind == 'c3' else 'ctd', Ci, Co)
        dx, part, amx = Out(N, H, W, Ci), Out(blocks, Ci, 2), Out(blocks, Ci)
        sa = (None, dz_blockmax(c).data_ptr(), 37) if blockmax else (dz_scalar(L, c).data_ptr(), None, 0)
        entry(dev(c.dz).data_ptr(), wpd.data_ptr(), dx.ptr(), *sa, zf.data_ptr(), mu.data_ptr(), isd.data_ptr(), ga.data_ptr(),
              be.data_ptr(), part.ptr(), amx.ptr(), N, H, W, Ci, Co, None)
        same(dx.np(), c.dx, 'dx (%s)' % ('integer' if sums else 'two-digit'))
        if sums:
            p = part.np().astype(np.float64).sum(0)
            same(p[:, 0], r.s1, 'sum dy')
            same(p[:, 1], r.s2, 'sum dy xhat')
            same(amx.np().max(0), r.amax, 'max |dy|')


# ------------------------------------------------------------------------------------------------------- dz formed on load
def _dzin_dgrad(L, c, rows, dz_out=False, front=None):
    N, H, W, Ci, Co = c.shape
    wpd, _ = pack16(L, c.K, 'c3d', Ci, Co)
    dx, dzo, part, amx = Out(N, H, W, Ci), Out(N, H, W, Co), Out(rows, Ci, 2), Out(rows, Ci)
    red = (None,) * 7
    if front is not None:
        zf, bn = front[:2]
        red = tuple(dev(a).data_ptr() for a in (zf, bn.mean, bn.invstd, bn.gamma, bn.beta)) + (part.ptr(), amx.ptr())
    L.dc_conv3x3_dgrad_dzin_f16x3(dev(c.da).data_ptr(), dev(c.zb).data_ptr(), dev(c.coef).data_ptr(), wpd.data_ptr(), dx.ptr(),
                                  dzo.ptr() if dz_out else None, *red, N, H, W, Ci, Co, None)
    return dx, dzo, part, amx


def _check_front(part, amx, front):
    p = part.np().astype(np.float64).sum(0)
    same(p[:, 0], front[2], 'sum dy')
    same(p[:, 1], front[3], 'sum dy xhat')
    same(amx.np().max(0), front[4], 'max |dy|')


@pytest.mark.parametrize('shape', lt.DZIN_DGRAD, ids=ids)
def test_conv3x3_dgrad_dzin_f16x3(dclib, shape):
    """dx with D = 0 (a real ReLU gate) and with D != 0 (z reaches dz as its lo digit); dz_out (more than 32 GEMM columns)
    equals dz; on integers the fused sums of the layer in front (red_z)."""
    L = dclib
    N, H, W, Ci, Co = shape
    rows = L.dc_conv3x3_dgrad_dzin_blocks(N, H, W, Ci, Co)
    if rows == 0:
        assert not _fused_paths_enabled()
        pytest.skip('role-split kernel switched off by an A/B knob')
    for with_D in (False, True):
        c = lt.dzin_case(*shape, with_D)
        dx, _, part, amx = _dzin_dgrad(L, c, rows)
        same(dx.np(), c.dx, 'dx, D %s 0' % ('!=' if with_D else '=='))
        assert np.isnan(part.np()).all() and np.isnan(amx.np()).all()
        if Ci > 32:
            dx, dzo, _, _ = _dzin_dgrad(L, c, rows, dz_out=True)
            same(dx.np(), c.dx, 'dx with dz_out')
            same(dzo.np(), c.dz, 'dz_out')
    c = lt.dzin_case(*shape, False, False)
    front = lt.front_sums(c)
    dx, _, part, amx = _dzin_dgrad(L, c, rows, front=front)
    same(dx.np(), c.dx, 'dx, integers')
    _check_front(part, amx, front)


@pytest.mark.parametrize('shape', lt.DZIN_WGRAD, ids=ids)
def test_conv3x3_wgrad_dzin_f16x3(dclib, shape):
    """dW from dz formed on load: x materialised with D = 0, x with BN + ReLU on load with D != 0."""
    L = dclib
    N, H, W, Ci, Co = shape
    for kw in (dict(with_D=False), dict(with_D=True, bnin=True)):
        c = lt.dzin_case(*shape, **kw)
        dw = Out(3, 3, Ci, Co)
        ws = torch.empty(L.dc_conv3x3_wgrad_ws_floats(N, H, W, Ci, Co), device='cuda')
        on_load = (dev(c.in_scale).data_ptr(), dev(c.in_shift).data_ptr()) if kw.get('bnin') else (None, None)
        L.dc_conv3x3_wgrad_dzin_f16x3(dev(c.x_raw).data_ptr(), *on_load, None, dev(c.da).data_ptr(), dev(c.zb).data_ptr(),
                                      dev(c.coef).data_ptr(), dw.ptr(), ws.data_ptr(), N, H, W, Ci, Co, None)
        same(dw.np(), c.dK, 'dW %r' % (kw,))


@pytest.mark.parametrize('shape', lt.DZIN_C1, ids=ids)
def test_first_layer_wgrad_dzin_and_z_rebuilt(dclib, shape):
    """Cin == 1 (fp32 FMA kernels: integer image, two-digit da): dc_conv3x3_wgrad_dzin_f16x3 from the stored z, and -- W % 4 == 0 --
    dc_conv3x3_c1_wgrad_dzin_zre from a z it rebuilds from (x, w, bias)."""
    L = dclib
    N, H, W, Ci, Co = shape
    c = lt.dzin_case(*shape, False, x_int=True)
    xd = dev(c.x.reshape(N, H, W))
    ws = torch.empty(L.dc_conv3x3_wgrad_ws_floats(N, H, W, 1, Co), device='cuda')
    dw = Out(3, 3, 1, Co)
    L.dc_conv3x3_wgrad_dzin_f16x3(xd.data_ptr(), None, None, None, dev(c.da).data_ptr(), dev(c.zb).data_ptr(), dev(c.coef).data_ptr(),
                                  dw.ptr(), ws.data_ptr(), N, H, W, 1, Co, None)
    same(dw.np(), c.dK, 'dW from the stored z')
    if W % 4:
        return
    r = lt.zre_case(N, H, W, Co)
    dw2 = Out(3, 3, 1, Co)
    L.dc_conv3x3_c1_wgrad_dzin_zre(xd.data_ptr(), dev(r.w).data_ptr(), dev(r.bias).data_ptr(), dev(c.da).data_ptr(), dev(c.coef).data_ptr(),
                                   dw2.ptr(), ws.data_ptr(), N, H, W, Co, None)
    same(dw2.np(), r.dK, 'dW from the rebuilt z')


def _joint(L, c, rows, bnin=False, front=None, rank_one=False):
    N, H, W, Ci, Co = c.shape
    wpd, _ = pack16(L, c.K, 'c3d', Ci, Co)
    dx, dw, part, amx = Out(N, H, W, Ci), Out(3, 3, Ci, Co), Out(rows, Ci, 2), Out(rows, Ci)
    ws = torch.empty(L.dc_conv3x3_bwd_joint_ws_floats(N, H, W, Ci, Co), device='cuda')
    xd = dev(c.x_raw)
    red = (None,) * 7
    if front is not None:
        bn = front[1]
        red = (xd.data_ptr(),) + tuple(dev(a).data_ptr() for a in (bn.mean, bn.invstd, bn.gamma, bn.beta)) + (part.ptr(), amx.ptr())
    on_load = (dev(c.in_scale).data_ptr(), dev(c.in_shift).data_ptr()) if bnin else (None, None)
    head = (xd.data_ptr(),) + on_load + (None,)
    tail = (dev(c.zb).data_ptr(), dev(c.coef).data_ptr(), wpd.data_ptr(), dx.ptr()) + red + (dw.ptr(), ws.data_ptr(), N, H, W, Ci, Co, None)
    if rank_one:
        L.dc_conv3x3_bwd_joint_r1_f16x3(*(head + (dev(c.s).data_ptr(), dev(c.kh).data_ptr()) + tail))
    else:
        L.dc_conv3x3_bwd_joint_f16x3(*(head + (dev(c.da).data_ptr(),) + tail))
    return dx, dw, part, amx


@pytest.mark.parametrize('shape', lt.JOINT, ids=ids)
def test_conv3x3_bwd_joint_f16x3(dclib, shape):
    """32 -> 32 and 64 -> 32: dx and dW with D = 0 and D != 0; 32 -> 32 also with x formed on load and, on integers, the sums of
    the layer in front whose pre-BN tensor is x itself."""
    L = dclib
    N, H, W, Ci, Co = shape
    rows = L.dc_conv3x3_bwd_joint_blocks(N, H, W, Ci, Co)
    if rows == 0:
        assert not _fused_paths_enabled()
        pytest.skip('joint backward switched off by an A/B knob')
    variants = [dict(with_D=False), dict(with_D=True)] + ([dict(with_D=False, bnin=True)] if Ci == 32 else [])
    for kw in variants:
        c = lt.dzin_case(*shape, **kw)
        dx, dw, _, _ = _joint(L, c, rows, bnin=kw.get('bnin', False))
        same(dx.np(), c.dx, 'dx %r' % (kw,))
        same(dw.np(), c.dK, 'dW %r' % (kw,))
    if Ci == 32:
        c = lt.dzin_case(*shape, False, False)
        front = lt.front_sums(c, x_is_front=True)
        dx, dw, part, amx = _joint(L, c, rows, front=front)
        same(dx.np(), c.dx, 'dx, integers')
        same(dw.np(), c.dK, 'dW, integers')
        _check_front(part, amx, front)


def test_conv3x3_bwd_joint_r1_f16x3(dclib):
    """Rank-one da = kd[c] s[pix] formed on load: two-digit s (dx, dW), integer s (dx, dW and the sums of the layer in front)."""
    L = dclib
    shape = lt.JOINT[0]
    rows = L.dc_conv3x3_bwd_joint_blocks(*shape)
    if rows == 0:
        assert not _fused_paths_enabled()
        pytest.skip('joint backward switched off by an A/B knob')
    c = lt.dzin_case(*shape, False, rank_one=True)
    dx, dw, _, _ = _joint(L, c, rows, rank_one=True)
    same(dx.np(), c.dx, 'dx')
    same(dw.np(), c.dK, 'dW')
    c = lt.dzin_case(*shape, False, False, rank_one=True)
    front = lt.front_sums(c, x_is_front=True)
    dx, dw, part, amx = _joint(L, c, rows, front=front, rank_one=True)
    same(dx.np(), c.dx, 'dx, integers')
    same(dw.np(), c.dK, 'dW, integers')
    _check_front(part, amx, front)


# --------------------------------------------------------------------- role-split instantiations at an uneven item count
def _cus():
    """the batch sizes below follow from the CU count; tests/test_lattice.py proves the cases of a whole MI355X"""
    n = torch.cuda.get_device_properties(0).multi_processor_count
    assert n == lt.MI355X_CUS, 'not the CU count the CPU module proved the uneven-items cases for'
    return n


def _family(H, W, Ncols):
    """N that gives the persistent launch between 1 and 2 items per workgroup, not a multiple of 8 (tests/_tileplan.py)"""
    found = tp.persistent_family(1, _cus(), H, W, Ncols)
    assert found is not None
    return found[0]


@pytest.mark.parametrize('inst', ['<2,2>', '<4,1>'])
def test_pp_forward_uneven_items_two_digit(dclib, inst):
    L = dclib
    H, W, Ci, Co = lt.PP_FWD[inst]
    N = _family(H, W, Co)
    if L.dc_conv3x3_pp_blocks(N, H, W, Ci, Co, 0, 0) == 0:
        assert not _fused_paths_enabled()
        pytest.skip('role-split kernel switched off by an A/B knob')
    assert L.dc_conv3x3_pp_blocks(N, H, W, Ci, Co, 0, 0) > 0
    c = lt.conv_case('c3', N, H, W, Ci, Co)
    sc, sh, y = lt.epilogue(c)
    wp, _ = pack16(L, c.K, 'c3f', Ci, Co)
    z, cat = Out(N, H, W, Co), Out(N, H, W, Co + 4)
    xd, bd = dev(c.x), dev(c.bias)
    L.dc_conv3x3_fwd_f16x3(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), z.ptr(), Co, None, 0, None, None, 0, None, 0, None, 0, None,
                           N, H, W, Ci, Co, None)
    L.dc_conv3x3_fwd_f16x3(xd.data_ptr(), wp.data_ptr(), bd.data_ptr(), cat.ptr(4), Co + 4, None, 0, dev(sc).data_ptr(), dev(sh).data_ptr(), 1,
                           None, 0, None, 0, None, N, H, W, Ci, Co, None)
    same(z.np(), c.z, 'z')
    same(strided(cat.np(), 4, Co, 'epilogue'), y, 'fused epilogue')


@pytest.mark.parametrize('inst', ['<2,2>', '<4,1>'])
def test_pp_dgrad_uneven_items_two_digit(dclib, inst):
    """plain data gradient and the dz-on-load one through the role-split kernel"""
    L = dclib
    H, W, Ci, Co = lt.PP_DGRAD[inst]
    N = _family(H, W, Ci)
    rows = L.dc_conv3x3_dgrad_dzin_blocks(N, H, W, Ci, Co)
    if L.dc_conv3x3_pp_blocks(N, H, W, Ci, Co, 1, 0) == 0 or rows == 0:
        assert not _fused_paths_enabled()
        pytest.skip('role-split kernel switched off by an A/B knob')
    assert L.dc_conv3x3_pp_blocks(N, H, W, Ci, Co, 1, 0) > 0 and rows > 0
    c = lt.conv_case('c3', N, H, W, Ci, Co)
    wpd, _ = pack16(L, c.K, 'c3d', Ci, Co)
    dx = Out(N, H, W, Ci)
    L.dc_conv3x3_dgrad_f16x3(dev(c.dz).data_ptr(), wpd.data_ptr(), dx.ptr(), dz_scalar(L, c).data_ptr(), None, 0, None, N, H, W, Ci, Co, None)
    same(dx.np(), c.dx, 'dx')
    d = lt.dzin_case(N, H, W, Ci, Co, False)
    dx, _, _, _ = _dzin_dgrad(L, d, rows)
    same(dx.np(), d.dx, 'dx, dz on load')


@pytest.mark.parametrize('Ci', [32, 64])
def test_bwd_joint_uneven_items_two_digit(dclib, Ci):
    L = dclib
    H, W = lt.JOINT_HW
    found = tp.persistent_family(1, _cus(), H, W)
    assert found is not None
    N = found[0]
    rows = L.dc_conv3x3_bwd_joint_blocks(N, H, W, Ci, 32)
    if rows == 0:
        assert not _fused_paths_enabled()
        pytest.skip('joint backward switched off by an A/B knob')
    assert rows > 0
    c = lt.dzin_case(N, H, W, Ci, 32, False)
    dx, dw, _, _ = _joint(L, c, rows)
    same(dx.np(), c.dx, 'dx')
    same(dw.np(), c.dK, 'dW')
