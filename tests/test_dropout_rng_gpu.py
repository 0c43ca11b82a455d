"""Production dropout (mask == NULL: keep-bits from the counter hash of csrc/common.h) against an independent restatement.

Every entry point that takes (mask, keep, seed) runs twice on the same inputs: once with mask = NULL and seed = s, once with
mask = oracle.hash_keep_mask(s, ...) uploaded and seed = 0.  Every output buffer must be BIT-equal (the kernels evaluate the same
expressions on a factor that is 0 or 1/keep either way), untouched columns of strided buffers included.  seed = s + 1 must give
another result, or the comparison would prove nothing.  The hash is indexed by the element of the DENSE tensor (pixel * C +
channel): the strided cases (ld = 2C, 3C, the engine's concat layouts) are where an ld / C mix-up would show.  Where the
forward output allows it the device's keep-bits are also read back directly (all-ones input) and compared with the host's, so a
failure says which side is off.  No tolerance anywhere in this file."""
import numpy as np
import pytest

from oracle import unet_numpy as on

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

SEED = 0xC2B2AE3D27D4EB4F          # > 2^63: the seed travels as an unsigned 64-bit value
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


def nans(*shape):
    return torch.full(shape, float('nan'), device='cuda')


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def biteq(a, b):
    """torch.equal on the bit patterns (NaN pre-fill of untouched columns compares equal to itself)."""
    return torch.equal(bits(a), bits(b))


def make(N, H, W, C, ldm, seed=0):
    """Inputs of every op below for a [N,H,W,C] BatchNorm layer (and a [N,H,W,C] up-sampling source); strided tensors are
    [.., ld] buffers whose LAST C columns are the tensor."""
    rs = np.random.RandomState(1000 * C + 10 * H + ldm + seed)
    f = np.float32
    ld = ldm * C
    d = dict(N=N, H=H, W=W, C=C, ld=ld, off=ld - C)
    d['z'] = rs.standard_normal((N, H, W, C)).astype(f)
    d['da'] = rs.standard_normal((N, H, W, ld)).astype(f)
    d['mean'] = (rs.standard_normal(C) * 0.2).astype(f)
    d['invstd'] = rs.uniform(0.5, 1.5, C).astype(f)
    d['gamma'] = (rs.uniform(0.5, 1.5, C) * rs.choice([-1.0, 1.0], C)).astype(f)
    d['beta'] = rs.uniform(-0.3, 0.3, C).astype(f)
    d['dgamma'] = rs.standard_normal(C).astype(f)
    d['dbeta'] = rs.standard_normal(C).astype(f)
    d['dout'] = rs.standard_normal((N, 2 * H, 2 * W, ld)).astype(f)
    if H % 2 == 0 and W % 2 == 0:
        d['dyp'] = rs.standard_normal((N, H // 2, W // 2, C)).astype(f)
        d['idx'] = rs.randint(0, 4, (N, H // 2, W // 2, C)).astype(np.uint8)
    return d


def second_half(d):
    """The inputs of the second half of the batch (a data-parallel rank's shard)."""
    n = d['N'] // 2
    h = dict(d, N=n)
    for k, v in d.items():
        if isinstance(v, np.ndarray) and v.ndim == 4:
            h[k] = v[n:]
    return h


def bn_ptrs(d):
    return [dev(d[k]).data_ptr() for k in ('mean', 'invstd', 'gamma', 'beta')]


# ---- the eight entry points: op(L, d, mask_ptr, keep, seed, count) -> [(name, tensor)], the first one depends on the bits ----
def op_fwd(L, d, mptr, keep, seed, count):
    N, H, W, C, ld, off = (d[k] for k in ('N', 'H', 'W', 'C', 'ld', 'off'))
    out, ab = nans(N, H, W, ld), nans(C)
    L.dc_bn_relu_drop_fwd(dev(d['z']).data_ptr(), *bn_ptrs(d), mptr, keep, seed, out.data_ptr() + 4 * off, ld, N * H * W, C,
                          float(count), ab.data_ptr(), None)
    return [('out', out), ('abound', ab)]


def op_pool_fwd(L, d, mptr, keep, seed, count):
    N, H, W, C, ld, off = (d[k] for k in ('N', 'H', 'W', 'C', 'ld', 'off'))
    out, ab, pooled = nans(N, H, W, ld), nans(C), nans(N, H // 2, W // 2, C)
    idx = torch.full((N, H // 2, W // 2, C), 255, dtype=torch.uint8, device='cuda')
    L.dc_bn_relu_drop_pool_fwd(dev(d['z']).data_ptr(), *bn_ptrs(d), mptr, keep, seed, out.data_ptr() + 4 * off, ld,
                               pooled.data_ptr(), idx.data_ptr(), N, H, W, C, float(count), ab.data_ptr(), None)
    return [('out', out), ('pooled', pooled), ('idx', idx), ('abound', ab)]


def op_bwd_reduce(L, d, mptr, keep, seed, count):
    N, H, W, C, ld, off = (d[k] for k in ('N', 'H', 'W', 'C', 'ld', 'off'))
    blocks = L.dc_bn_bwd_blocks(N * H * W, C)
    part, amax = nans(blocks, C, 2), nans(blocks, C)
    L.dc_bn_bwd_reduce(dev(d['da']).data_ptr() + 4 * off, ld, dev(d['z']).data_ptr(), *bn_ptrs(d), mptr, keep, seed,
                       part.data_ptr(), amax.data_ptr(), N * H * W, C, None)
    return [('partial', part), ('amax_partial', amax)]


def _apply(L, d, mptr, keep, seed, count, with_count):
    N, H, W, C, ld, off = (d[k] for k in ('N', 'H', 'W', 'C', 'ld', 'off'))
    blocks = L.dc_bn_bwd_blocks(N * H * W, C)
    dz, dbp, amax = nans(N, H, W, C), nans(blocks, C), nans(blocks)
    head = (dev(d['da']).data_ptr() + 4 * off, ld, dev(d['z']).data_ptr(), *bn_ptrs(d), mptr, keep, seed,
            dev(d['dgamma']).data_ptr(), dev(d['dbeta']).data_ptr(), dz.data_ptr(), dbp.data_ptr(), amax.data_ptr(), N * H * W)
    if with_count:
        L.dc_bn_bwd_apply_count(*head, float(count), C, None)
    else:
        L.dc_bn_bwd_apply(*head, C, None)
    return [('dz', dz), ('dbias_partial', dbp), ('absmax_partial', amax)]


def op_bwd_apply(L, d, mptr, keep, seed, count):
    return _apply(L, d, mptr, keep, seed, count, False)


def op_bwd_apply_count(L, d, mptr, keep, seed, count):
    return _apply(L, d, mptr, keep, seed, count, True)


def op_pool_bwd_bnred(L, d, mptr, keep, seed, count):
    N, H, W, C, ld, off = (d[k] for k in ('N', 'H', 'W', 'C', 'ld', 'off'))
    blocks = L.dc_maxpool2x2_bwd_blocks(N, H, W, C)
    dx, part, amax = nans(N, H, W, C), nans(blocks, C, 2), nans(blocks, C)
    L.dc_maxpool2x2_bwd_bnred(dev(d['dyp']).data_ptr(), dev(d['idx']).data_ptr(), dev(d['da']).data_ptr() + 4 * off, ld,
                              dx.data_ptr(), dev(d['z']).data_ptr(), *bn_ptrs(d), mptr, keep, seed, part.data_ptr(),
                              amax.data_ptr(), N, H, W, C, None)
    return [('bn_partial', part), ('amax_partial', amax), ('dx', dx)]


def op_up_fwd(L, d, mptr, keep, seed, count):
    N, H, W, C, ld, off = (d[k] for k in ('N', 'H', 'W', 'C', 'ld', 'off'))
    out, ab = nans(N, 2 * H, 2 * W, ld), nans(C)
    L.dc_upsample2x_drop_fwd(dev(d['z']).data_ptr(), out.data_ptr() + 4 * off, ld, mptr, keep, seed,
                             dev(np.abs(d['beta']) + 1).data_ptr(), 0, ab.data_ptr(), 0, N, H, W, C, None)
    return [('out', out), ('abound_out', ab)]


def op_up_bwd(L, d, mptr, keep, seed, count):
    N, H, W, C, ld, off = (d[k] for k in ('N', 'H', 'W', 'C', 'ld', 'off'))
    din = nans(N, H, W, C)
    L.dc_upsample2x_drop_bwd(dev(d['dout']).data_ptr() + 4 * off, ld, mptr, keep, seed, din.data_ptr(), N, H, W, C, None)
    return [('din', din)]


BN_OPS = {'dc_bn_relu_drop_fwd': op_fwd, 'dc_bn_bwd_reduce': op_bwd_reduce, 'dc_bn_bwd_apply': op_bwd_apply,
          'dc_bn_bwd_apply_count': op_bwd_apply_count}
POOL_OPS = {'dc_bn_relu_drop_pool_fwd': op_pool_fwd, 'dc_maxpool2x2_bwd_bnred': op_pool_bwd_bnred}
UP_OPS = {'dc_upsample2x_drop_fwd': op_up_fwd, 'dc_upsample2x_drop_bwd': op_up_bwd}
ALL_OPS = dict(BN_OPS, **POOL_OPS, **UP_OPS)


def masked_elems(name, d):
    """Elements of the dense tensor the dropout of `name` acts on."""
    up = 4 if name in UP_OPS else 1
    return up * d['N'] * d['H'] * d['W'] * d['C']


def check_rng_equals_mask(L, name, d, keep, seed, mask=None):
    op = ALL_OPS[name]
    count = 2 * d['N'] * d['H'] * d['W']          # only dc_bn_bwd_apply_count's dz and the abound outputs depend on it
    if mask is None:
        mask = on.hash_keep_mask(seed, masked_elems(name, d), keep)
    assert 0 < int(mask.sum()) < mask.size
    rng = op(L, d, None, keep, seed, count)
    exp = op(L, d, dev(mask).data_ptr(), keep, 0, count)
    other = op(L, d, None, keep, (seed + 1) & (2 ** 64 - 1), count)
    torch.cuda.synchronize()
    for (what, a), (_, b) in zip(rng, exp):
        assert biteq(a, b), '%s: %s differs between RNG(seed) and the uploaded hash_keep_mask(seed)' % (name, what)
    assert not biteq(rng[0][1], other[0][1]), '%s: seed + 1 gave the same %s' % (name, rng[0][0])
    # strided outputs: the tensor's columns are all written, the others all untouched
    for what, a in rng:
        if what == 'out' and d['off']:
            a = a.cpu().numpy()
            assert np.isnan(a[..., :d['off']]).all() and not np.isnan(a[..., d['off']:]).any()
        elif what != 'out':
            assert not torch.isnan(a.float()).any(), (name, what)
    return rng


# the last case of each list has more work than the kernel's grid cap covers in one round (the grid-stride loop wraps)
# C = 4 (one quad per pixel) .. 512; 1x12x20 and 3x7x9: pixel counts that are no multiple of the pixels per block; ld = C, 2C, 3C
BN_CASES = [(2, 16, 16, 4, 1, 0.75), (1, 12, 20, 4, 3, 0.5), (3, 7, 9, 8, 2, 0.75), (1, 12, 20, 8, 3, 0.5), (3, 7, 9, 32, 3, 0.5),
            (1, 12, 20, 32, 2, 0.75), (3, 7, 9, 256, 2, 0.75), (1, 12, 20, 256, 1, 0.5), (3, 7, 9, 512, 1, 0.75), (1, 12, 20, 512, 2, 0.5),
            (4, 40, 44, 256, 2, 0.75)]
POOL_CASES = [(1, 12, 20, 4, 2, 0.75), (2, 16, 16, 4, 1, 0.5), (1, 12, 20, 8, 3, 0.5), (1, 12, 20, 32, 2, 0.75), (2, 6, 10, 256, 3, 0.75),
              (1, 12, 20, 256, 1, 0.5), (1, 12, 20, 512, 2, 0.75), (2, 2, 6, 512, 3, 0.5), (8, 64, 80, 256, 1, 0.5)]
# up-sampling SOURCE shapes (the dropout acts on [N,2H,2W,C]); 3x80x72x64: 4 320 > 4 096 blocks, the forward's grid-stride loop wraps
UP_CASES = [(1, 6, 10, 4, 2, 0.75), (3, 7, 9, 4, 1, 0.5), (3, 7, 9, 8, 3, 0.5), (1, 6, 10, 32, 2, 0.75), (3, 7, 9, 256, 3, 0.75),
            (1, 6, 10, 256, 1, 0.5), (1, 6, 10, 512, 2, 0.5), (3, 7, 9, 512, 3, 0.75), (3, 80, 72, 64, 1, 0.5), (3, 80, 72, 64, 2, 0.75)]


@pytest.mark.parametrize('name', sorted(BN_OPS))
@pytest.mark.parametrize('N,H,W,C,ldm,keep', BN_CASES)
def test_bn_dropout_rng_equals_host_mask(dclib, name, N, H, W, C, ldm, keep):
    check_rng_equals_mask(dclib, name, make(N, H, W, C, ldm), keep, SEED + C)


@pytest.mark.parametrize('name', sorted(POOL_OPS))
@pytest.mark.parametrize('N,H,W,C,ldm,keep', POOL_CASES)
def test_pooling_dropout_rng_equals_host_mask(dclib, name, N, H, W, C, ldm, keep):
    check_rng_equals_mask(dclib, name, make(N, H, W, C, ldm), keep, SEED + C)


@pytest.mark.parametrize('name', sorted(UP_OPS))
@pytest.mark.parametrize('N,H,W,C,ldm,keep', UP_CASES)
def test_upsample_dropout_rng_equals_host_mask(dclib, name, N, H, W, C, ldm, keep):
    check_rng_equals_mask(dclib, name, make(N, H, W, C, ldm), keep, SEED + C)


def test_upsample_bwd_grid_stride_wraps(dclib):
    """dc_upsample2x_drop_bwd runs one thread per SOURCE quad: 3 x 160 x 144 x 64 is 4 320 > 4 096 blocks."""
    check_rng_equals_mask(dclib, 'dc_upsample2x_drop_bwd', make(3, 160, 144, 64, 1), 0.5, SEED)


@pytest.mark.parametrize('name', sorted(ALL_OPS))
@pytest.mark.parametrize('keep', [0.75, 0.5])
def test_sharded_seed_draws_the_whole_batch_bits(dclib, name, keep):
    """A data-parallel rank runs its shard under parallel.shard_drop_seed(s, n, r): rank 1's launch on the second half of a batch
    must equal the same launch under the second half of the WHOLE batch's host mask -- and, for the outputs that are a function
    of their own element only, the second half of the whole-batch launch."""
    from deep_calcium_amd import parallel
    L = dclib
    N, H, W, C, ldm = 4, 6, 10, 32, 2
    whole = make(N, H, W, C, ldm)
    half = second_half(whole)
    n = masked_elems(name, half)
    s1 = parallel.shard_drop_seed(SEED, n, 1)
    assert s1 != SEED
    wmask = on.hash_keep_mask(SEED, 2 * n, keep)
    got = check_rng_equals_mask(L, name, half, keep, s1, mask=wmask[n:])
    # `count` of check_rng_equals_mask's half launch = 2 * its pixels = the whole batch's pixels
    ref = ALL_OPS[name](L, whole, None, keep, SEED, N * H * W)
    torch.cuda.synchronize()
    elementwise = {'dc_bn_relu_drop_fwd': ('out', 'abound'), 'dc_bn_relu_drop_pool_fwd': ('out', 'pooled', 'idx', 'abound'),
                   'dc_bn_bwd_apply_count': ('dz',), 'dc_maxpool2x2_bwd_bnred': ('dx',), 'dc_upsample2x_drop_fwd': ('out', 'abound_out'),
                   'dc_upsample2x_drop_bwd': ('din',)}.get(name, ())
    for (what, a), (_, b) in zip(got, ref):
        if what in elementwise:
            assert biteq(a, b[N // 2:] if b.dim() == 4 else b), (name, what)
    # rank 1 under the UNSHARDED seed would repeat rank 0's bits
    same = ALL_OPS[name](L, half, None, keep, SEED, N * H * W)
    torch.cuda.synchronize()
    assert not biteq(got[0][1], same[0][1])


@pytest.mark.parametrize('C,ldm,keep', [(4, 1, 0.75), (8, 3, 0.5), (32, 2, 0.75), (256, 2, 0.5), (512, 3, 0.75)])
def test_device_keep_bits_read_back_equal_the_host_hash(dclib, C, ldm, keep):
    """All-ones input through identity BatchNorm (mean 0, invstd 1, gamma 1, beta 0): output > 0 <=> kept.  The bits of the three
    forward kernels are compared with hash_keep_mask element by element; the up-sampling backward of an all-ones gradient at
    keep = 0.5 returns 2 x (kept elements of the 2x2 block), exactly."""
    L = dclib
    N, H, W = 1, 12, 20
    d = make(N, H, W, C, ldm)
    one, zero = np.ones(C, np.float32), np.zeros(C, np.float32)
    d.update(z=np.ones((N, H, W, C), np.float32), mean=zero, invstd=one, gamma=one, beta=zero)
    seed = SEED ^ C
    want = on.hash_keep_mask(seed, N * H * W * C, keep).reshape(N, H, W, C)
    want_up = on.hash_keep_mask(seed, 4 * N * H * W * C, keep).reshape(N, 2 * H, 2 * W, C)
    for name, ref in (('dc_bn_relu_drop_fwd', want), ('dc_bn_relu_drop_pool_fwd', want), ('dc_upsample2x_drop_fwd', want_up)):
        out = ALL_OPS[name](L, d, None, keep, seed, N * H * W)[0][1]
        torch.cuda.synchronize()
        o = out.cpu().numpy()[..., d['off']:]
        assert set(np.unique(o)) == {np.float32(0), np.float32(1) / np.float32(keep)}, name
        assert np.array_equal((o > 0).astype(np.uint8), ref), name
    d['dout'] = np.ones((N, 2 * H, 2 * W, d['ld']), np.float32)
    want05 = on.hash_keep_mask(seed, 4 * N * H * W * C, 0.5).reshape(N, H, 2, W, 2, C)
    din = op_up_bwd(L, d, None, 0.5, seed, 0)[0][1]
    torch.cuda.synchronize()
    assert np.array_equal(din.cpu().numpy(), 2.0 * want05.sum((2, 4), dtype=np.float32))
