"""The UNet1D training kernels at production tile counts and grids, against float64, through the C ABI.

The direct tests (test_spikes_gpu.py, test_spikes_train_gpu.py) run every 1-D kernel where production (batch 20, 4096 frames,
nfb 32) never is: ONE tile per weight-gradient workgroup and at most 12 slabs, forward grids of 8 workgroups or fewer (where the
XCD-first map of blockIdx.x is the identity), the two vector reductions below their grid caps.  This module enters the other side:

  * dc_conv1d_k5_wgrad (wgrad.hip, all four instantiations of CONV1D_WGRAD_DISPATCH) at 2 / 3 / 5 / 6 tiles per workgroup: both
    LDS tiles staged again behind the trailing barrier, accumulation across tiles, tile ranges that run from one trace into the
    next, a short last split, a ragged last tile of a trace in the middle of a range, ragged channel blocks, and 64 slabs or more
    (dc_reduce_partials' two-stage path) -- case table and its CPU proof: tests/_tileplan.py WGRAD1D_CASES, tests/test_tileplan.py;
  * dc_conv1d_k5_fwd (spikes.hip), forward and as the data gradient, on grids of 20 to 48 workgroups, multiples of 8 and not;
  * dc_conv1d_stats and dc_conv1d_k5_c1_wgrad (spikes_train.hip) past STATS_MAX_BLOCKS / C1W_MAX_BLOCKS: 17 and 33 trips a lane.

Inputs, references and tolerances are the direct tests': random fp32 operands, the float64 oracles of _unet1d_ref.py and
_unet1d_train_ref.py, max |error| <= 1e-4 * max |reference|; outputs are prefilled with POISON; a dirty workspace or partial buffer
may change no bit.  Every test prints the figure it asserts on.

Would a wrong kernel fail?  A tile that is dropped, added twice or read from the wrong place changes the weight gradient by that
tile's own contribution.  test_conv1d_k5_wgrad_multitile_probes is built so that this is the WHOLE gradient's size: dz is zero but
at nine samples placed on the tile, split and trace boundaries, and the test itself asserts (on the float64 side) that leaving any
one of them out moves the reference by more than 5 % of its maximum -- 500 times the tolerance.  For the random rows the same
figure, max |ref - ref without one tile| / max |ref|, was computed in float64 on the CPU for EVERY tile of the smallest size of
each row (the ragged last tile of a trace; every tile where T = 5); its minimum over those tiles, per row in table order:

    32x32  3.6e-02 3.6e-02 7.2e-03 9.2e-03      64x32  1.2e-01 6.3e-02 3.4e-02 5.9e-02
    32x64  1.2e-01 6.7e-02 2.5e-02 5.5e-02      64x64  1.1e-01 1.7e-01 4.1e-02 4.9e-02 1.9e-02

-- 72 to 1700 times the 1e-4 bound (the smallest: a 20-sample tile of (103, 1300, 4, 12); the 2-sample tile of (7, 450, 768, 256):
4.9e-02), so no single tile of any row can go missing within the tolerance.

Measured on an MI355X when the module was written, beside the 1e-4 bound: weight gradient, worst row per instantiation 1.8e-07
(32x32), 1.8e-07 (64x32), 1.6e-07 (32x64), 4.3e-07 (64x64), probes 8.8e-08; forward grids 1.2e-06, data gradient 1.3e-06; statistics
3.1e-14 (double partials), first-layer weight gradient 8.9e-08."""
import functools

import numpy as np
import pytest

import _tileplan as tp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _unet1d_train_ref as tref       # noqa: E402
import test_spikes_gpu as sg           # noqa: E402  _conv_inputs, _conv_ref (the float64 _unet1d_ref.conv1d_k5), _run_conv
import test_spikes_train_gpu as tr     # noqa: E402  _run_wgrad, GRAD_SHAPES, the device helpers

POISON, _st, _dev, _empty, _rel = tr.POISON, tr._st, tr._dev, tr._empty, tr._rel
TOL = 1e-4          # the project's parity contract, as in test_conv1d_k5_wgrad / test_conv1d_k5_fwd


def _x(s):
    return 'x'.join(map(str, s))


def test_the_direct_tests_are_the_shapes_proven_single_tile():
    """tests/_tileplan.py's copy of test_conv1d_k5_wgrad's shapes (proven on the CPU to run one tile per workgroup) is current."""
    shapes = [m.args[1] for m in tr.test_conv1d_k5_wgrad.pytestmark if m.name == 'parametrize']
    assert len(shapes) == 1 and list(shapes[0]) == tp.WGRAD1D_DIRECT_SHAPES
    assert tr.GRAD_SHAPES == tp.WGRAD1D_DIRECT_SHAPES[:len(tr.GRAD_SHAPES)]


# ---- weight gradient at several tiles per workgroup --------------------------------------------------------------------------
def wgrad_inputs(shape):
    """Random fp32 (x, dz) as test_spikes_train_gpu._conv_case draws them (not kept: the table's operands add up to 150 MB)."""
    N, T, Cin, Cout = shape
    rs = np.random.RandomState(N * 1000 + T + Cin + Cout)
    x = rs.randn(N, T, Cin).astype(np.float32)
    k = (rs.randn(5, Cin, Cout) * np.sqrt(2. / (5 * Cin))).astype(np.float32)
    dz = rs.randn(N, T, Cout).astype(np.float32)
    return x, k, dz


def _wg_id(c):
    return '%s-%s-%dt' % (c[0], _x(c[1:5]), c[5])


@pytest.mark.parametrize('case', tp.WGRAD1D_CASES, ids=_wg_id)
def test_conv1d_k5_wgrad_multitile(dclib, case):
    inst, N, T, Cin, Cout, tps, last = case
    plan = tp.wgrad1d_plan(N, T, Cin, Cout)
    splits = plan[7]
    assert (plan[0], plan[6], plan[8]) == (inst, tps, last) and tps > 1
    # the mirror against the library
    assert dclib.dc_conv1d_k5_wgrad_blocks(N, T, Cin, Cout) == splits
    assert dclib.dc_conv1d_k5_wgrad_ws_floats(N, T, Cin, Cout) >= (splits + 32) * 5 * Cin * Cout
    x, k, dz = wgrad_inputs((N, T, Cin, Cout))
    _, want = tref.conv_grads(x, k, dz)
    got = tr._run_wgrad(dclib, x, dz, 0.)               # dw prefilled with POISON, the workspace with 0
    err = _rel(got, want)
    print('dc_conv1d_k5_wgrad %s %r: %d tiles, %d per workgroup, %d slabs (last %d): %.3g'
          % (inst, (N, T, Cin, Cout), plan[5], tps, splits, last, err))
    assert np.isfinite(got).all() and err <= TOL
    # a dirty workspace changes no bit: every slab written, summed in a fixed order
    assert np.array_equal(got, tr._run_wgrad(dclib, x, dz, 1e30))


def wgrad_probes(N, T, Cin, Cout):
    """The probed samples {name: (trace, sample)} of a probe row and the traces (before, after) whose x is made huge, from the
    mirror alone."""
    inst, TW, CM, CN, per, total, tps, splits, last = tp.wgrad1d_plan(N, T, Cin, Cout)

    def tile(t):                                        # -> trace, first sample, samples
        n, j = divmod(t, per)
        return n, j * TW, min(TW, T - j * TW)

    probes = {}
    # the last tile of all: ragged, the last of the SHORT last split
    n, t0, cnt = tile(total - 1)
    assert last < tps and cnt < TW and (total - 1) // tps == splits - 1 and (n, t0 + cnt - 1) == (N - 1, T - 1)
    probes['last sample of the last tile'] = (n, t0 + cnt - 1)
    # the first tile of a trace that is the second or later tile of its workgroup, and the (ragged) tile before it
    k = next(k for k in range(1, N - 1) if (k * per) % tps != 0)
    tb = k * per
    assert tile(tb)[:2] == (k, 0) and tb // tps == (tb - 1) // tps and tb - (tb // tps) * tps >= 1
    probes['first sample of a trace, mid-range'] = (k, 0)
    n, t0, cnt = tile(tb - 1)
    assert (n, t0 + cnt - 1) == (k - 1, T - 1) and cnt < TW
    probes['last sample of the tile before it'] = (n, t0 + cnt - 1)
    # a trace in the middle: its two ends (the halo must stop there) and a tile boundary inside it (the halo must NOT stop)
    m = N // 2
    assert {m - 1, m, m + 1}.isdisjoint({k - 1, k, N - 1}) and per > 1
    probes['sample 0 of a middle trace'] = (m, 0)
    probes['sample T-1 of a middle trace'] = (m, T - 1)
    probes['last sample of its first tile'] = (m, TW - 1)
    probes['first sample of its second tile'] = (m, TW)
    # the same tile boundary in a trace whose tiles 0 and 1 belong to DIFFERENT workgroups: the halo comes from global memory,
    # whatever the previous workgroup staged
    j = next(j for j in range(2, N - 1) if (j * per + 1) % tps == 0 and j not in (m - 1, m, m + 1, k - 1, k))
    probes['last sample of a range'] = (j, TW - 1)
    probes['first sample of the next range'] = (j, TW)
    return probes, (m - 1, m + 1)


@pytest.mark.parametrize('case', tp.WGRAD1D_PROBE_CASES, ids=_wg_id)
def test_conv1d_k5_wgrad_multitile_probes(dclib, case):
    """dz is zero but at nine samples on the tile, range and trace boundaries the mirror names; the gradient is then the sum of
    nine outer products, each of the size of the whole -- a dropped, doubled or misplaced tile is an error of order one."""
    inst, N, T, Cin, Cout, tps, last = case
    probes, (before, after) = wgrad_probes(N, T, Cin, Cout)
    rs = np.random.RandomState(T + Cin)
    x = rs.randn(N, T, Cin).astype(np.float32)
    x[before, T - 4:] = 1e6                             # what a halo read past the middle trace's ends would pick up
    x[after, :4] = 1e6
    dz = np.zeros((N, T, Cout), np.float32)
    solo = {}
    for name, (n, t) in probes.items():
        dz[n, t] = rs.choice([-1., 1.], Cout) * rs.uniform(0.5, 1.5, Cout)
        c = np.zeros((5, Cin, Cout))
        for tap in range(5):
            u = t + tap - 2
            if 0 <= u < T:                              # x is ZERO outside [0, T) of its own trace
                c[tap] = np.outer(x[n, u].astype(np.float64), dz[n, t].astype(np.float64))
        solo[name] = c
    assert len({p for p in probes.values()}) == len(probes) == 9
    want = sum(solo.values())
    scale = np.abs(want).max()
    assert scale < 100.                                 # nothing of the 1e6 neighbours belongs in it
    for name, c in solo.items():                        # by design: without any one probed sample the reference is another
        assert np.abs(c).max() >= 0.05 * scale, name
    got = tr._run_wgrad(dclib, x, dz, 1e30)
    assert np.isfinite(got).all()
    err = _rel(got, want)
    print('dc_conv1d_k5_wgrad probes %s %r: %.3g; probes %r' % (inst, (N, T, Cin, Cout), err, sorted(probes.values())))
    assert err <= TOL


# ---- forward and data gradient on grids past 8 workgroups --------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fwd_case(shape):
    N, T, Cin, Cout = shape
    x, k, scale, shift = sg._conv_inputs(N, T, Cin, Cout, seed=N + T + Cin + Cout)
    want = sg._conv_ref(x, k, scale, shift, 0)          # relu = 1: np.maximum(want, 0), which is what _conv_ref does
    for a in (x, k, scale, shift, want):
        a.setflags(write=False)
    return x, k, scale, shift, want


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('shape,grid', tp.CONV1D_FWD_CASES, ids=lambda v: _x(v) if isinstance(v, tuple) else 'g%d' % v)
def test_conv1d_k5_fwd_large_grids(dclib, shape, grid, relu):
    N, T, Cin, Cout = shape
    assert tp.conv1d_fwd_grid(N, T, Cout) == grid
    x, k, scale, shift, want = fwd_case(shape)
    want = np.maximum(want, 0.) if relu else want
    got = sg._run_conv(dclib, x, k, scale, shift, relu)             # the output prefilled with POISON
    assert np.isfinite(got).all() and not (got == POISON).any()
    err = np.abs(got - want).max() / np.abs(want).max()
    print('dc_conv1d_k5_fwd %r relu=%d, %d workgroups (%d mod 8): max err / max |ref| = %.3g' % (shape, relu, grid, grid % 8, err))
    assert err <= TOL


FWD_EXTRA = [(3, 260, 36, 136), (5, 130, 8, 72), (2, 70, 256, 768)]


@pytest.mark.parametrize('shape', FWD_EXTRA, ids=_x)
def test_conv1d_k5_fwd_large_grids_slice_and_batching(dclib, shape):
    N, T, Cin, Cout = shape
    assert shape in [s for s, _ in tp.CONV1D_FWD_CASES] and tp.conv1d_fwd_grid(N, T, Cout) > 8
    x, k, scale, shift, _ = fwd_case(shape)
    dense = sg._run_conv(dclib, x, k, scale, shift, 1)
    # into the channel slice [2 Cout, 3 Cout) of a wider buffer: the same bits, nothing else written
    got = sg._run_conv(dclib, x, k, scale, shift, 1, y_ld=3 * Cout, chan0=2 * Cout)
    assert (got[..., :2 * Cout] == POISON).all() and np.array_equal(got[..., 2 * Cout:], dense)
    # the batching invariance the kernel documents: a trace alone (another grid, another workgroup map) gives the same bits
    for n in range(N):
        alone = sg._run_conv(dclib, x[n:n + 1], k, scale, shift, 1)
        assert np.array_equal(alone[0], dense[n]), n


@pytest.mark.parametrize('shape', FWD_EXTRA, ids=_x)
def test_data_gradient_on_large_grids(dclib, shape):
    """The route of test_data_gradient_is_the_forward_on_repacked_weights: the layer is Cout -> Cin of the forward shape, its dx
    the forward kernel on dz with the weights packed flipped and transposed, scale 1, shift 0 -- the same grid as the table's."""
    N, T, Cz, Cx = shape                                # dz has the forward shape's Cin channels, dx its Cout
    assert tp.conv1d_fwd_grid(N, T, Cx) > 8
    rs = np.random.RandomState(N + T + Cz)
    x = rs.randn(N, T, Cx).astype(np.float32)
    k = (rs.randn(5, Cx, Cz) * np.sqrt(2. / (5 * Cx))).astype(np.float32)
    dz = rs.randn(N, T, Cz).astype(np.float32)
    dx_want, _ = tref.conv_grads(x, k, dz)
    kd, wp = _dev(k), _empty(k.size)
    dclib.dc_pack_weights(kd.data_ptr(), wp.data_ptr(), 5, Cz, Cx, Cx * Cz, 1, Cz, 1, _st())        # flipped, Cin <-> Cout
    ones, zeros = torch.ones(Cx, device='cuda'), torch.zeros(Cx, device='cuda')
    dzd, dx = _dev(dz), _empty(N * T * Cx)
    dclib.dc_conv1d_k5_fwd(dzd.data_ptr(), wp.data_ptr(), ones.data_ptr(), zeros.data_ptr(), 0, dx.data_ptr(), Cx, N, T, Cz, Cx, _st())
    torch.cuda.synchronize()
    got = dx.cpu().numpy().reshape(N, T, Cx)
    err = _rel(got, dx_want)
    print('data gradient %r, %d workgroups: %.3g' % (shape, tp.conv1d_fwd_grid(N, T, Cx), err))
    assert np.isfinite(got).all() and err <= TOL


# ---- the two vector reductions past their grid caps --------------------------------------------------------------------------
def test_conv1d_stats_past_the_grid_cap(dclib):
    C, pixels = 1024, 16384 + 37                        # one sample lane a block: nothing smaller reaches 1024 blocks x 16 samples
    blocks = dclib.dc_conv1d_stats_blocks(pixels, C)
    assert blocks == 1024 and tp.quad_plan(pixels, C, 16, 1024) == (1024, 17)          # the cap; the longest lane runs 17 trips
    z = np.random.default_rng(5).standard_normal((pixels, C), dtype=np.float32) * np.float32(2.) + np.float32(3.)
    zd = _dev(z)
    outs = []
    for fill in (0., 7.):
        part = torch.full((blocks, C, 2), fill, dtype=torch.float64, device='cuda')
        dclib.dc_conv1d_stats(zd.data_ptr(), C, part.data_ptr(), pixels, C, _st())
        torch.cuda.synchronize()
        outs.append(part.cpu().numpy())
    assert np.array_equal(outs[0], outs[1])             # every row written, the same bits twice
    want = np.stack([z.sum(0, dtype=np.float64), np.einsum('pc,pc->c', z, z, dtype=np.float64)], 1)
    err = _rel(outs[0].sum(0), want)
    print('dc_conv1d_stats (%d, %d), %d blocks, 17 trips: %.3g' % (pixels, C, blocks, err))
    assert err <= 1e-4                                  # test_conv1d_stats' bound


def test_conv1d_k5_c1_wgrad_past_the_grid_cap(dclib):
    N, T, Cout = 3, 5477, 1024                          # 16431 samples > 512 blocks x 32 samples of the one lane a block has
    assert tp.quad_plan(N * T, Cout, 32, 512) == (512, 33)
    n_ws = dclib.dc_conv1d_k5_c1_wgrad_ws_floats(N, T, Cout)
    assert n_ws == (512 + 32) * 5 * Cout                # 512 slabs + the reduce kernel's second-stage scratch
    rs = np.random.RandomState(T)
    x = rs.randn(N, T, 1).astype(np.float32)
    k = rs.randn(5, 1, Cout).astype(np.float32)
    dz = np.random.default_rng(T).standard_normal((N, T, Cout), dtype=np.float32)
    _, want = tref.conv_grads(x, k, dz)
    xd, dzd = _dev(x), _dev(dz)
    outs = []
    for fill in (0., 1e30):
        dw, ws = _empty(5 * Cout), _empty(n_ws, fill)
        dclib.dc_conv1d_k5_c1_wgrad(xd.data_ptr(), dzd.data_ptr(), dw.data_ptr(), ws.data_ptr(), N, T, Cout, _st())
        torch.cuda.synchronize()
        outs.append(dw.cpu().numpy().reshape(5, 1, Cout))
    err = _rel(outs[0], want)
    print('dc_conv1d_k5_c1_wgrad %r, 512 blocks, 33 trips: %.3g' % ((N, T, Cout), err))
    assert err <= 1e-4 and np.array_equal(outs[0], outs[1])         # test_conv1d_k5_c1_wgrad's bound and its dirty-workspace check
