"""Exact-lattice data for the matrix kernels (numpy only): inputs on which every convolution result is ONE exactly known
number per element whatever the order of summation, so a GPU test can compare with np.array_equal.

A two-digit lattice number is 0 or (D1 + D0 * 2^-12) * m: D1 a non-zero integer in +-{1, 2}, D0 in {-1, 0, 1}, m a power of
two.  Under any power-of-two scale s the split-fp16 kernels' hi = fp16(v s) is D1 m s and lo = fp16(v s - hi) is D0 2^-12 m s,
both exact; hi*hi and the two cross products are multiples of g = 2^-12 (times the scales), and the lo*lo product -- the only
term off that grid -- is dropped by definition.  While the per-element sum of |a| |b| over the contraction stays below
2^24 g, every partial sum in any order is a multiple of g below 2^24 g and fp32 holds it exactly.

The split (csrc/f16x3_common.h dc_split_f16), the weight scale of the pack (csrc/igemm_f16x3.hip pack_split_body) and the two
power-of-two guards (csrc/common.h dc_pow2_guard, dc_pow2_from_absmax) are RESTATED here from their definitions."""
import functools
import zlib
from types import SimpleNamespace as NS

import numpy as np

from oracle import unet_numpy as on

G = 2.0 ** -12
LIMIT = 2.0 ** 24
F16_MIN_NORMAL = 2.0 ** -14
GRAD = 2.0 ** -20          # magnitude of the gradient operands (dz of a mean loss over ~1e6 elements)


# ---------------------------------------------------------------------------------------------------------------- generator
def _seed(*key):
    return zlib.crc32(repr(key).encode()) & 0x7fffffff


def lattice(rs, shape, density=1.0, lo=True, positive=False, mult=1.0):
    """0 (share 1 - density) or (D1 + D0 2^-12) mult; lo=False: the single-digit (integer) kind."""
    d1 = rs.randint(1, 3, shape).astype(np.float64)
    if not positive:
        d1 *= rs.choice([-1.0, 1.0], shape)
    d0 = rs.randint(-1, 2, shape).astype(np.float64) if lo else 0.0
    keep = rs.random_sample(shape) < density
    v = np.where(keep, d1 + d0 * G, 0.0) * mult
    out = v.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), v)
    return out


def digits(v, mult=1.0):
    """(D1, D0) of lattice values; asserts that they are lattice values with a non-zero leading digit (or 0)."""
    u = np.asarray(v, np.float64) / mult
    d1 = np.round(u)
    d0 = (u - d1) / G
    assert np.array_equal(d0, np.round(d0)) and np.abs(d0).max(initial=0) <= 2, 'not a two-digit lattice number'
    assert np.all((d1 != 0) | (u == 0)), 'a value without its leading digit would go into hi entirely'
    return d1, d0


# ------------------------------------------------------------------------------------------- the kernels' rules, restated
def split_f16(x, s=1.0):
    """hi = fp16(x s), lo = fp16(x s - hi): s a power of two, so x s is exact in fp32 and the device's single-rounding
    fma form gives these bits."""
    s = np.float32(s)
    assert s > 0 and np.log2(float(s)) == np.round(np.log2(float(s)))
    xs = np.asarray(x, np.float32) * s
    assert np.array_equal(xs.astype(np.float64), np.asarray(x, np.float64) * float(s))
    hi = xs.astype(np.float16)
    lo = (xs - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def halves(x, s=1.0):
    """(hi, lo) / s in float64.  Asserts what the construction rests on: hi + lo is x exactly, and every half as the kernel
    stages it is an fp16 NORMAL number or 0 (nothing here depends on fp16 subnormals in the matrix unit)."""
    hi, lo = split_f16(x, s)
    h, l = hi.astype(np.float64), lo.astype(np.float64)
    assert np.array_equal(h + l, np.asarray(x, np.float64) * float(s)), 'split not exact'
    for a in (np.abs(h), np.abs(l)):
        assert np.all((a == 0) | ((a >= F16_MIN_NORMAL) & (a <= 65504.0))), 'operand half outside the fp16 normal range'
    return h / float(s), l / float(s)


def lo_share(x, s=1.0):
    """share of the non-zero values that carry a non-zero lo digit"""
    _, l = halves(x, s)
    nz = np.asarray(x) != 0
    return float((l[nz] != 0).mean()) if nz.any() else 0.0


def _floor_log2(m):
    return int(np.floor(np.log2(float(m))))


def weight_scale(w):
    """pack_split_body: 2^(10 - floor(log2 max|w|)), max|w| * scale in [2^10, 2^11); 1 for all-zero kernels."""
    amax = np.float32(np.abs(np.asarray(w, np.float32)).max())
    return 2.0 ** (10 - _floor_log2(amax)) if amax > 0 else 1.0


def guard_scale(bound):
    """dc_pow2_guard on the largest per-channel bound: brings it into [2^14, 2^15); None -> 1."""
    if bound is None:
        return 1.0
    m = np.float32(np.abs(np.asarray(bound, np.float32)).max())
    return 2.0 ** (14 - _floor_log2(m)) if m > 0 else 1.0


def absmax_scale(m, target=1024.0):
    """dc_pow2_from_absmax: 2^floor(log2(target / m)) in fp32."""
    m = np.float32(m)
    if not m > 0:
        return 1.0
    r = np.float32(target) / m
    e = np.floor(np.log2(r, dtype=np.float32))
    assert float(r) == 2.0 ** float(e) or abs(float(np.log2(float(r))) - np.round(np.log2(float(r)))) > 1e-4, 'log2f on a knife edge'
    return 2.0 ** float(np.clip(e, -100, 100))


def pack_image(w_flat, taps, K, Ncols, s_tap, s_k, s_n, flip):
    """The split-fp16 weight image [tap][K/8][hi|lo][n][8] and its trailer (scale, max|w|) from the rules above."""
    flat = np.asarray(w_flat, np.float32).ravel()
    ws = weight_scale(flat)
    K8 = (K + 7) // 8
    img = np.zeros((taps, K8, 2, Ncols, 8), np.float16)
    n = np.arange(Ncols)
    for tap in range(taps):
        ts = taps - 1 - tap if flip else tap
        for k in range(K):
            hi, lo = split_f16(flat[ts * s_tap + k * s_k + n * s_n], ws)
            img[tap, k // 8, 0, :, k % 8] = hi
            img[tap, k // 8, 1, :, k % 8] = lo
    return img.ravel(), np.float32(ws), np.float32(np.abs(flat).max())


# --------------------------------------------------------------------------------------------------- the float64 operations
def _z(*shape):
    return np.zeros(shape, np.float64)


def op_c3_fwd(x, K):
    return on.conv3x3_fwd(x, K, 0.0)


def op_c3_dgrad(dz, K):
    return on.conv3x3_bwd(_z(*dz.shape[:3], K.shape[2]), K, dz)[0]


def op_c3_wgrad(x, dz):
    return on.conv3x3_bwd(x, _z(3, 3, x.shape[3], dz.shape[3]), dz)[1]


def op_ct_fwd(x, K):
    return on.convT2x2_fwd(x, K, 0.0)


def op_ct_dgrad(dz, K):
    return on.convT2x2_bwd(_z(dz.shape[0], dz.shape[1] // 2, dz.shape[2] // 2, K.shape[3]), K, dz)[0]


def op_ct_wgrad(x, dz):
    return on.convT2x2_bwd(x, _z(2, 2, dz.shape[3], x.shape[3]), dz)[1]


def op_c1d_fwd(x, K):
    """Conv1D(k=5, 'same'): x [N,T,Ci], K [5,Ci,Co]"""
    N, T, Ci = x.shape
    xp = np.zeros((N, T + 4, Ci))
    xp[:, 2:-2] = x
    return sum(xp[:, t:t + T] @ K[t] for t in range(5))


def op_c1d_wgrad(x, dz):
    N, T, Ci = x.shape
    xp = np.zeros((N, T + 4, Ci))
    xp[:, 2:-2] = x
    return np.stack([xp[:, t:t + T].reshape(-1, Ci).T @ dz.reshape(-1, dz.shape[2]) for t in range(5)])


def f64(a):
    return np.asarray(a, np.float64)


def exact32(a):
    """the float64 array is exactly representable in fp32"""
    a = f64(a)
    return np.array_equal(a.astype(np.float32).astype(np.float64), a)


def units(op, a, b, unit):
    """largest per-element sum of |a| |b| over the contraction, in units of the grid: the exactness condition is < 2^24"""
    return float(op(np.abs(f64(a)), np.abs(f64(b))).max() / unit)


def expected3(op, a, sa, b, sb):
    """sum (a_hi b_hi + a_hi b_lo + a_lo b_hi) by linearity: op(a, b) - op(a_lo, b_lo); float64 is exact on these dyadic
    operands (products on the grid 2^-24, sums far below 2^53 of it)."""
    _, al = halves(a, sa)
    _, bl = halves(b, sb)
    return op(f64(a), f64(b)) - op(al, bl)


def brute_c3_fwd_units(x, sx, K, sk, pix, co):
    """One output element of the conv3x3 forward as a Python-int sum in units of g^2 = 2^-24 (hi, lo are integers there), with
    the lo*lo products left out -- the brute-force cross-check of expected3."""
    xh, xl = halves(x, sx)
    kh, kl = halves(K, sk)
    n, oy, ox = pix
    _, H, W, Ci = x.shape
    U = 2 ** 24
    tot = 0
    for a in range(3):
        for c in range(3):
            y, xx = oy + a - 1, ox + c - 1
            if not (0 <= y < H and 0 <= xx < W):
                continue
            for ci in range(Ci):
                ah, al = int(round(xh[n, y, xx, ci] * 4096)), int(round(xl[n, y, xx, ci] * 4096))
                bh, bl = int(round(kh[a, c, ci, co] * 4096)), int(round(kl[a, c, ci, co] * 4096))
                tot += ah * bh + ah * bl + al * bh
    return tot / U


# ---------------------------------------------------------------------------------------------------------------- the cases
CONV3 = [   # N, H, W, Cin, Cout
    (1, 8, 8, 16, 32),          # the premise case: one tile, one K-chunk
    (1, 20, 36, 8, 24),         # ragged: partial tiles, Cin < chunk, Cout % 32 != 0
    (2, 40, 40, 144, 96),       # ragged in y, x and columns
    (1, 24, 48, 136, 64),       # partial last chunk (Cin % 16 = 8)
    (3, 12, 12, 200, 96),       # split-K with a partial tile and a partial last chunk
    (1, 8, 8, 512, 512),        # split-K on 8 x 8 tiles (N = 1 still splits: asserted on the device)
    (1, 16, 16, 256, 256),      # split-K at 16 x 16
]
PREMISE = CONV3[0]
CONVT = [(1, 10, 18, 16, 8), (1, 16, 16, 128, 64), (2, 33, 64, 32, 96), (1, 4, 4, 512, 256)]
MEAN_UNITS = 2.0 ** 23      # the densities aim the MEAN per-element sum of |a| |b| at half the limit; the check is on the max


def _densities(terms_fwd, terms_dgrad, terms_wgrad, g):
    """densities of (x, dz); the weights stay dense.  E|v|^2 = 2.25 for D1 in +-{1, 2}.  Lower density, never fewer cases."""
    cap = MEAN_UNITS * g / 2.25 / 2.0
    dx = min(1.0, cap / terms_fwd)
    dd = min(1.0, cap / terms_dgrad)
    if terms_wgrad * dx * dd > cap:
        f = np.sqrt(cap / (terms_wgrad * dx * dd))
        dx, dd = dx * f, dd * f
    return dx, dd


@functools.lru_cache(maxsize=None)
def conv_case(kind, N, H, W, Ci, Co, two_digit=True, grad=GRAD, with_abound=False):
    """Inputs, scales and expected values of the three contractions of a conv3x3 ('c3') or conv-transpose ('ct') layer.
    two_digit: the split-fp16 expected value (lo*lo dropped); else integers, where fp32 and split-fp16 agree with plain sums."""
    taps = 9 if kind == 'c3' else 1
    rs = np.random.RandomState(_seed(kind, N, H, W, Ci, Co, two_digit))
    g = G if two_digit else 1.0
    # integer cases keep the same limit with g = 1: the sums are far below it at full density
    dx, dd = _densities(taps * Ci, taps * Co, N * H * W, G) if two_digit else (1.0, 1.0)
    c = NS(kind=kind, shape=(N, H, W, Ci, Co), two_digit=two_digit, g=g, grad=grad, dens=(dx, dd))
    Ho, Wo = (H, W) if kind == 'c3' else (2 * H, 2 * W)
    c.x = lattice(rs, (N, H, W, Ci), dx, two_digit)
    c.K = lattice(rs, (3, 3, Ci, Co) if kind == 'c3' else (2, 2, Co, Ci), 1.0, two_digit)
    c.dz = lattice(rs, (N, Ho, Wo, Co), dd, two_digit, mult=grad)
    c.bias = rs.randint(-3, 4, Co).astype(np.float32)
    # the scales the kernels derive: weight trailer, gradient scale from max|dz| (target 1024), activation guard
    c.s_k = weight_scale(c.K)
    c.s_dz = absmax_scale(np.abs(c.dz).max())
    c.abound = np.abs(c.x).reshape(-1, Ci).max(0).astype(np.float32) if with_abound else None
    c.s_x = guard_scale(c.abound)
    fwd, dgrad, wgrad = (op_c3_fwd, op_c3_dgrad, op_c3_wgrad) if kind == 'c3' else (op_ct_fwd, op_ct_dgrad, op_ct_wgrad)
    c.units = dict(fwd=units(fwd, c.x, c.K, g) + np.abs(c.bias).max() / g, dgrad=units(dgrad, c.dz, c.K, g * grad),
                   wgrad=units(wgrad, c.x, c.dz, g * grad))
    assert max(c.units.values()) < LIMIT, c.units
    if two_digit:
        c.z = expected3(fwd, c.x, c.s_x, c.K, c.s_k) + f64(c.bias)
        c.dx = expected3(dgrad, c.dz, c.s_dz, c.K, c.s_k)
        c.dK = expected3(wgrad, c.x, c.s_x, c.dz, c.s_dz)
        c.lo = dict(x=lo_share(c.x, c.s_x), K=lo_share(c.K, c.s_k), dz=lo_share(c.dz, c.s_dz))
    else:
        for a, s in ((c.x, c.s_x), (c.K, c.s_k), (c.dz, c.s_dz)):
            assert not halves(a, s)[1].any()              # single digit: no lo half
        c.z = fwd(f64(c.x), f64(c.K)) + f64(c.bias)
        c.dx = dgrad(f64(c.dz), f64(c.K))
        c.dK = wgrad(f64(c.x), f64(c.dz))
    assert exact32(c.z) and exact32(c.dx) and exact32(c.dK)
    return c


def epilogue(c):
    """The fused forward epilogue on the exact z: relu(z scale + shift), power-of-two scale, integer shift."""
    Co = c.shape[4]
    rs = np.random.RandomState(Co + 5)
    sc = rs.choice([0.5, 1.0, 2.0], Co).astype(np.float32)
    sh = rs.randint(-2, 3, Co).astype(np.float32)
    y = np.maximum(c.z * f64(sc) + f64(sh), 0.0)
    assert exact32(c.z * f64(sc)) and exact32(y)           # same bits whether the compiler contracts v*sc + sh or not
    return sc, sh, y


def maxpool(y):
    N, H, W, C = y.shape
    return y.reshape(N, H // 2, 2, W // 2, 2, C).max((2, 4))


# -- BatchNorm + ReLU on load --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bnin_case(kind, N, H, W, Ci, Co):
    """The consumer forms a = relu(fmaf(z_in, in_scale, in_shift)) while staging.  in_scale in {+-1, +-2}, integer in_shift
    (positive in at least one channel: zero padding must stay zero, relu(shift) must not leak into the border); z_in is
    chosen so that a is again 0 or a two-digit number: the expected values are conv_case's with x := a."""
    taps = 9 if kind == 'c3' else 1
    rs = np.random.RandomState(_seed('bnin', kind, N, H, W, Ci, Co))
    dx, dd = _densities(taps * Ci, taps * Co, N * H * W, G)
    c = NS(kind=kind, shape=(N, H, W, Ci, Co), two_digit=True, g=G, grad=GRAD, dens=(dx, dd))
    a = lattice(rs, (N, H, W, Ci), dx, True, positive=True)
    below = -lattice(rs, (N, H, W, Ci), 0.5, True, positive=True)          # what the ReLU cuts: negative or 0
    pre = np.where(a != 0, a, below).astype(np.float64)
    c.in_scale = rs.choice([1.0, -1.0, 2.0, -2.0], Ci).astype(np.float32)
    c.in_shift = rs.randint(-2, 4, Ci).astype(np.float32)
    c.in_shift[0] = 3.0
    zin = (pre - f64(c.in_shift)) / f64(c.in_scale)
    c.z_in = zin.astype(np.float32)
    assert np.array_equal(f64(c.z_in), zin)
    y = f64(c.z_in) * f64(c.in_scale) + f64(c.in_shift)                   # fmaf: one rounding of an exact value
    assert exact32(y)
    c.x = np.maximum(y, 0.0).astype(np.float32)
    assert np.array_equal(c.x, a) and (c.in_shift > 0).any()
    digits(c.x)
    c.K = lattice(rs, (3, 3, Ci, Co) if kind == 'c3' else (2, 2, Co, Ci), 1.0, True)
    Ho, Wo = (H, W) if kind == 'c3' else (2 * H, 2 * W)
    c.dz = lattice(rs, (N, Ho, Wo, Co), dd, True, mult=GRAD)
    c.s_k, c.s_dz = weight_scale(c.K), absmax_scale(np.abs(c.dz).max())
    c.abound = np.full(Ci, 2.0 + G, np.float32)                           # bounds every channel of a
    c.s_x = guard_scale(c.abound)
    fwd, wgrad = (op_c3_fwd, op_c3_wgrad) if kind == 'c3' else (op_ct_fwd, op_ct_wgrad)
    c.units = dict(fwd=units(fwd, c.x, c.K, G), wgrad=units(wgrad, c.x, c.dz, G * GRAD))
    assert max(c.units.values()) < LIMIT, c.units
    c.z = expected3(fwd, c.x, c.s_x, c.K, c.s_k)
    c.dK = expected3(wgrad, c.x, c.s_x, c.dz, c.s_dz)
    c.lo = dict(x=lo_share(c.x, c.s_x), K=lo_share(c.K, c.s_k), dz=lo_share(c.dz, c.s_dz))
    assert exact32(c.z) and exact32(c.dK)
    return c


# -- BatchNorm pass-1 sums of the layer in front ("bnred"): integer data -------------------------------------------------
def bn_layer(rs, C):
    """integer mean / gamma / beta, power-of-two invstd: dc_bn_affine and xhat are exact"""
    return NS(mean=rs.randint(-2, 3, C).astype(np.float32), invstd=rs.choice([0.5, 1.0, 2.0], C).astype(np.float32),
              gamma=rs.choice([-1.0, 1.0, 2.0], C).astype(np.float32), beta=rs.randint(-2, 3, C).astype(np.float32))


def bnred_expected(da, z, bn, da_unit=1.0):
    """(sum dy, sum dy xhat, max |dy|) per channel with the device's gate fmaf(z, gamma invstd, beta - mean gamma invstd) > 0;
    asserts the exactness condition of the fp32 sums (every term a multiple of the smallest invstd, sum |terms| < 2^24 of it)."""
    C = z.shape[-1]
    gsc = f64(bn.gamma) * f64(bn.invstd)
    gsh = f64(bn.beta) - f64(bn.mean) * gsc
    z2, da2 = f64(z).reshape(-1, C), f64(da).reshape(-1, C)
    dy = np.where(z2 * gsc + gsh > 0, da2, 0.0)
    xh = (z2 - f64(bn.mean)) * f64(bn.invstd)
    unit = da_unit * 0.5                                              # invstd >= 1/2
    assert np.array_equal(np.round(dy * xh / unit), dy * xh / unit)
    assert max(np.abs(dy).sum(0).max(), np.abs(dy * xh).sum(0).max()) / unit < LIMIT
    return dy.sum(0), (dy * xh).sum(0), np.abs(dy).max(0)


# -- dz formed on load ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dzin_case(N, H, W, Ci, Co, with_D, two_digit=True, bnin=False, x_int=False, rank_one=False):
    """dz = fmaf(A, dy, fmaf(D, z - mu, E)), dy = [fmaf(z, sc, sh) > 0] da, from a hand-written table (rows sc | sh | mu | A | D
    | E | bound).  with_D = False: D = 0, A in {1, -1, 2}, a real ReLU gate on integer z.  with_D = True: D = 2^-12, z = mu + D0,
    da = D1, gate open everywhere: the lo digit of dz arrives THROUGH z.  rank_one: da[p][c] = kd[c] s[p]."""
    rs = np.random.RandomState(_seed('dzin', N, H, W, Ci, Co, with_D, two_digit, bnin, x_int, rank_one))
    dx_, dd = _densities(9 * Ci, 9 * Co, N * H * W, G) if two_digit else (1.0, 1.0)
    if not two_digit:
        dd = min(1.0, 2.0 ** 21 / (N * H * W))                              # bn sums: sum |dy xhat| < 2^24 units
    c = NS(shape=(N, H, W, Ci, Co), two_digit=two_digit, g=G if two_digit else 1.0, with_D=with_D, dens=(dx_, dd))
    mu = rs.randint(-2, 3, Co).astype(np.float32)
    E = np.zeros(Co, np.float32)
    if with_D:
        assert two_digit and not rank_one
        v = lattice(rs, (N, H, W, Co), dd, True)
        d1, d0 = digits(v)
        c.da = d1.astype(np.float32)
        c.zb = (f64(mu) + d0).astype(np.float32)
        sc, sh = np.ones(Co, np.float32), np.full(Co, 8.0, np.float32)
        A, D = np.ones(Co, np.float32), np.full(Co, G, np.float32)
    else:
        A = rs.choice([1.0, -1.0, 2.0], Co).astype(np.float32)
        D = np.zeros(Co, np.float32)
        sc, sh = rs.choice([1.0, -1.0], Co).astype(np.float32), rs.randint(-1, 2, Co).astype(np.float32)
        c.zb = rs.randint(-3, 4, (N, H, W, Co)).astype(np.float32)
        if rank_one:
            c.s = lattice(rs, (N, H, W), min(1.0, 2 * dd), two_digit)
            c.kh = np.zeros((Co, 2), np.float32)
            c.kh[:, 0] = rs.randint(-1, 2, Co)
            kd = rs.choice([1.0, -1.0, 2.0, 0.0], Co)
            c.kh[:, 1] = c.kh[:, 0] + kd
            A = np.ones(Co, np.float32)
            c.da = (f64(c.s)[..., None] * kd).astype(np.float32)
        else:
            c.da = lattice(rs, (N, H, W, Co), dd, two_digit)
    y = f64(c.zb) * f64(sc) + f64(sh)
    dy = np.where(y > 0, f64(c.da), 0.0)
    inner = f64(D) * (f64(c.zb) - f64(mu)) + f64(E)
    dz = f64(A) * dy + inner
    assert exact32(inner) and exact32(dz)
    c.dz = dz.astype(np.float32)
    digits(c.dz)
    bound = np.full(Co, 8.0, np.float32)
    assert np.abs(c.dz).max() <= 8.0 and (y > 0).mean() > 0.3
    c.coef = np.stack([sc, sh, mu, A, D, E, bound]).astype(np.float32)
    c.s_dz = guard_scale(bound)
    # the block input: materialised, BN + ReLU on load, or the (N, H, W) image of the first layer (integers: fp32 FMA kernels)
    c.in_scale = c.in_shift = None
    if bnin:
        b = bnin_case('c3', N, H, W, Ci, Co)
        c.x_raw, c.x, c.in_scale, c.in_shift = b.z_in, b.x, b.in_scale, b.in_shift
        if not two_digit:
            raise ValueError('bnin cases are two-digit')
    else:
        c.x = lattice(rs, (N, H, W, Ci), dx_, two_digit and not x_int)
        c.x_raw = c.x
    c.K = lattice(rs, (3, 3, Ci, Co), 1.0, two_digit)
    c.s_k = weight_scale(c.K)
    c.units = dict(dgrad=units(op_c3_dgrad, c.dz, c.K, c.g), wgrad=units(op_c3_wgrad, c.x, c.dz, c.g))
    assert max(c.units.values()) < LIMIT, c.units
    c.dx = expected3(op_c3_dgrad, c.dz, c.s_dz, c.K, c.s_k)
    c.dK = expected3(op_c3_wgrad, c.x, 1.0, c.dz, c.s_dz)
    c.lo = dict(x=lo_share(c.x), K=lo_share(c.K, c.s_k), dz=lo_share(c.dz, c.s_dz))
    assert exact32(c.dx) and exact32(c.dK)
    return c


def joint_front_layer(c):
    """The layer in front of a 32 -> 32 joint backward, whose pre-BN tensor IS the block input x (integer cases): invstd 1, so
    that in_scale = gamma, in_shift = beta - mean gamma are the integers the on-load ReLU of x uses as well."""
    Ci = c.shape[3]
    rs = np.random.RandomState(Ci + 11)
    bn = bn_layer(rs, Ci)
    bn.invstd = np.ones(Ci, np.float32)
    return bn


# -- integer cases of the fp32 kernels without a split: first layer (Cin == 1) and the 1-D convolutions ------------------------
@functools.lru_cache(maxsize=None)
def c1_case(N, H, W, Co):
    rs = np.random.RandomState(_seed('c1', N, H, W, Co))
    c = NS(shape=(N, H, W, Co))
    c.x = lattice(rs, (N, H, W, 1), 1.0, False)
    c.K = lattice(rs, (3, 3, 1, Co), 1.0, False)
    c.bias = rs.randint(-3, 4, Co).astype(np.float32)
    c.dz = lattice(rs, (N, H, W, Co), min(1.0, 2.0 ** 20 / (N * H * W)), False)
    c.z = op_c3_fwd(f64(c.x), f64(c.K)) + f64(c.bias)
    c.dK = op_c3_wgrad(f64(c.x), f64(c.dz))
    c.units = dict(fwd=units(op_c3_fwd, c.x, c.K, 1.0) + 3, wgrad=units(op_c3_wgrad, c.x, c.dz, 1.0))
    assert max(c.units.values()) < LIMIT and exact32(c.z) and exact32(c.dK)
    return c


@functools.lru_cache(maxsize=None)
def conv1d_case(N, T, Ci, Co):
    """Conv1D(k=5, 'same') on integers; Ci == 1: the first layer, x the (N, T) trace matrix."""
    rs = np.random.RandomState(_seed('c1d', N, T, Ci, Co))
    c = NS(shape=(N, T, Ci, Co))
    c.x = lattice(rs, (N, T, Ci), 1.0, False)
    c.K = lattice(rs, (5, Ci, Co), 1.0, False)
    c.dz = lattice(rs, (N, T, Co), 1.0, False)
    c.scale = rs.choice([0.5, 1.0, 2.0], Co).astype(np.float32)
    c.shift = rs.randint(-3, 4, Co).astype(np.float32)
    acc = op_c1d_fwd(f64(c.x), f64(c.K))
    c.y = np.maximum(acc * f64(c.scale) + f64(c.shift), 0.0)
    c.dK = op_c1d_wgrad(f64(c.x), f64(c.dz))
    c.units = dict(fwd=units(op_c1d_fwd, c.x, c.K, 0.5) + 6, wgrad=units(op_c1d_wgrad, c.x, c.dz, 1.0))
    assert max(c.units.values()) < LIMIT and exact32(c.y) and exact32(c.dK)
    return c


@functools.lru_cache(maxsize=None)
def stats_case(kind, N, H, W, Ci, Co, tile_pixels, bnin=False):
    """Integer z small enough that the float64 BatchNorm partial rows are exact.  The rows are Chan merges, not plain sums, so
    a plain-sum bound does not apply: every lane forms shifted sums around its first value, and lanes, then waves, are merged
    with Chan's update in fp32 (csrc/common.h DcMoments); the row is (n mean, M2 + n mean^2) in double.  A merge is exact
    when both sides hold the SAME power-of-two count (weight 1/2) -- an 8 x 8 tile that lies inside the image: 64 pixels, a
    lane pair and at most two waves per column -- and the values fit: with integer |z| <= Z every mean is a multiple of 1/n
    below Z and every M2 a multiple of 1/n below 4 n Z^2, exact in fp32 while 4 n^2 Z^2 < 2^24, n = tile_pixels.  The rows then
    sum (in float64) to the integer sums of z and z^2.  kind 'ct': conv-transpose, 4 Cout columns per row.  bnin: x is formed
    on load from z_in with in_scale +-1 and an integer in_shift."""
    rs = np.random.RandomState(_seed('stats', kind, N, H, W, Ci, Co, bnin))
    c = NS(shape=(N, H, W, Ci, Co), two_digit=False, kind=kind)
    c.x = rs.choice([-1.0, 0.0, 1.0], (N, H, W, Ci), p=[0.05, 0.9, 0.05]).astype(np.float32)
    if bnin:
        c.x = np.abs(c.x)
        c.in_scale = rs.choice([1.0, -1.0], Ci).astype(np.float32)
        c.in_shift = rs.randint(-1, 3, Ci).astype(np.float32)
        c.in_shift[0] = 2.0
        pre = np.where(c.x != 0, f64(c.x), -f64(rs.randint(0, 3, c.x.shape)))        # what the ReLU cuts: <= 0
        c.z_in = ((pre - f64(c.in_shift)) / f64(c.in_scale)).astype(np.float32)
        assert np.array_equal(np.maximum(f64(c.z_in) * f64(c.in_scale) + f64(c.in_shift), 0.0), f64(c.x))
        c.abound = np.ones(Ci, np.float32)
    if kind == 'c3':
        c.K = rs.choice([-1.0, 0.0, 1.0], (3, 3, Ci, Co), p=[0.2, 0.6, 0.2]).astype(np.float32)
        c.z = op_c3_fwd(f64(c.x), f64(c.K))
    else:
        c.K = rs.choice([-1.0, 0.0, 1.0], (2, 2, Co, Ci), p=[0.3, 0.4, 0.3]).astype(np.float32)
        c.z = op_ct_fwd(f64(c.x), f64(c.K))
    Z = np.abs(c.z).max()
    assert tile_pixels & (tile_pixels - 1) == 0 and 4 * tile_pixels ** 2 * Z ** 2 < LIMIT, Z
    assert H % 8 == 0 and W % 8 == 0 and tile_pixels == 64 and (c.z != 0).mean() > 0.3
    c.units = dict(fwd=float(Z))
    c.sums = np.stack([c.z.sum((0, 1, 2)), (c.z ** 2).sum((0, 1, 2))], -1)
    return c


@functools.lru_cache(maxsize=None)
def c1_stats_case(N, H, W, Co):
    """dc_conv3x3_c1_fwd: a thread takes groups of 4 pixels (W % 4 == 0) and the 1024 / Cout pixel lanes of a block are merged
    ONE AFTER THE OTHER (weights 1/2, 1/3, 1/4, ...): dyadic only with at most two lanes, Cout >= 512.  Here every thread holds
    one group (n = 4), a row is the merge of two (n = 8) or stays empty; integers with 4 n^2 (2 Z)^2 < 2^24 (the shift of the
    sums is the bias plus the centre pixel times the kernel sum, |.| <= Z as well, so |v - K| <= 2 Z)."""
    assert W % 4 == 0 and 1024 // Co <= 2 and N * H * W // 4 <= 2 * ((N * H * W + 1024 // Co - 1) // (1024 // Co))
    rs = np.random.RandomState(_seed('c1stats', N, H, W, Co))
    c = NS(shape=(N, H, W, Co), two_digit=False)
    c.x = lattice(rs, (N, H, W, 1), 1.0, False)
    c.K = lattice(rs, (3, 3, 1, Co), 1.0, False)
    c.bias = rs.randint(-3, 4, Co).astype(np.float32)
    c.z = op_c3_fwd(f64(c.x), f64(c.K)) + f64(c.bias)
    Z = 2 * 18 + 3                                     # bound of |z| AND of the shift: 9 taps of |x| |w| <= 4, plus the bias
    assert np.abs(c.z).max() <= Z and 4 * 8 ** 2 * (2 * Z) ** 2 < LIMIT
    c.units = dict(fwd=float(Z))
    c.sums = np.stack([c.z.sum((0, 1, 2)), (c.z ** 2).sum((0, 1, 2))], -1)
    return c


@functools.lru_cache(maxsize=None)
def zre_case(N, H, W, Co):
    """dc_conv3x3_c1_wgrad_dzin_zre: z is REBUILT from the integer image, kernel and bias (exact), the table's gate then acts on
    that z; D = 0, two-digit da: x integer times dz two-digit -> every product a multiple of g."""
    c = dzin_case(N, H, W, 1, Co, False, x_int=True)
    rs = np.random.RandomState(_seed('zre', N, H, W, Co))
    r = NS(shape=(N, H, W, 1, Co), two_digit=True, base=c, x=c.x, da=c.da, coef=c.coef, s_dz=c.s_dz, s_k=1.0)
    r.w = lattice(rs, (3, 3, 1, Co), 1.0, False)
    r.K = r.w
    r.bias = rs.randint(-2, 3, Co).astype(np.float32)
    z = op_c3_fwd(f64(c.x), f64(r.w)) + f64(r.bias)
    sc, sh, A = (f64(c.coef[i]) for i in (0, 1, 3))
    dz = A * np.where(z * sc + sh > 0, f64(c.da), 0.0)
    assert exact32(z) and exact32(dz) and np.abs(dz).max() <= 8.0 and not c.coef[4].any() and not c.coef[5].any()
    r.z, r.dz = z, dz.astype(np.float32)
    digits(r.dz)
    r.units = dict(wgrad=units(op_c3_wgrad, c.x, r.dz, G))
    assert r.units['wgrad'] < LIMIT
    r.dK = op_c3_wgrad(f64(c.x), dz)                   # x has no lo half: nothing is dropped
    r.lo = dict(dz=lo_share(r.dz, r.s_dz))
    r.check = ('dz',)                                  # image and kernel are integers by design (fp32 FMA kernel)
    assert exact32(r.dK)
    return r


# ---- the case lists of tests/test_exact_conv_gpu.py (tests/test_lattice.py proves the conditions for every one of them) ------
INT_F32 = [('c3', 1, 20, 36, 8, 24), ('c3', 2, 40, 40, 144, 96), ('c3', 3, 12, 12, 200, 96), ('ct', 1, 10, 18, 16, 8), ('ct', 2, 33, 64, 32, 96)]
C1 = [(1, 20, 36, 8), (2, 32, 32, 32)]
CONV1D = [(2, 77, 8, 12), (1, 300, 36, 20), (3, 130, 64, 32)]
CONV1D_C1 = [(2, 77, 1, 12), (3, 300, 1, 32)]
BNIN = [('c3', 1, 20, 36, 8, 24), ('c3', 1, 24, 48, 136, 64), ('c3', 3, 12, 12, 200, 96), ('ct', 1, 10, 18, 16, 8), ('ct', 1, 16, 16, 128, 64)]
POOL = [(1, 40, 72, 48, 80), (2, 48, 64, 32, 32)]
BNRED = [('c3', 1, 40, 72, 48, 80), ('c3', 2, 48, 48, 32, 32), ('ct', 1, 20, 40, 128, 64), ('ct', 2, 17, 33, 256, 128)]
DZIN_DGRAD = [(2, 48, 48, 32, 32), (1, 40, 72, 48, 80)]                    # <4,1> and <2,2>, ragged
DZIN_WGRAD = [(1, 40, 72, 48, 32), (2, 16, 16, 64, 128), (2, 8, 8, 128, 64)]
DZIN_C1 = [(1, 17, 23, 1, 8), (2, 32, 32, 1, 32)]
JOINT = [(1, 40, 72, 32, 32), (1, 40, 72, 64, 32)]
STATS = [('c3', 2, 8, 8, 64, 256, 64, False), ('c3', 2, 8, 8, 64, 256, 64, True), ('ct', 2, 8, 8, 64, 64, 64, False),
         ('ct', 2, 8, 8, 64, 64, 64, True)]
C1_STATS = (1, 8, 8, 512)
ZRE = [(2, 32, 32, 32)]
GUARDED = [('c3', 1, 20, 36, 8, 24), ('ct', 1, 10, 18, 16, 8)]              # plain kernels under in_abound / x_abound
# role-split ("pp") instantiations at an uneven item count: H, W, Cin, Cout of tests/test_multitile_gpu.py; N from the CU count
PP_FWD = {'<2,2>': (12, 40, 64, 160), '<4,1>': (20, 40, 64, 32)}
PP_DGRAD = {'<2,2>': (12, 40, 160, 64), '<4,1>': (20, 40, 32, 64)}
JOINT_HW = (10, 40)
MI355X_CUS = 256


@functools.lru_cache(maxsize=None)
def bnred_case(kind, N, H, W, Ci, Co):
    """Integer data gradient whose output dx IS the `da` of the BatchNorm layer in front (pre-BN tensor zf, integers): the
    expected pass-1 sums and maxima of that layer."""
    c = conv_case(kind, N, H, W, Ci, Co, False)
    rs = np.random.RandomState(_seed('bnred', kind, N, H, W, Ci, Co))
    r = NS(conv=c, zf=rs.randint(-3, 4, (N, H, W, Ci)).astype(np.float32), bn=bn_layer(rs, Ci))
    r.s1, r.s2, r.amax = bnred_expected(c.dx, r.zf, r.bn, c.grad)
    return r


def front_sums(c, x_is_front=False):
    """dzin / joint integer case -> (zf, bn, s1, s2, amax) of the layer in front of its dx"""
    N, H, W, Ci, Co = c.shape
    rs = np.random.RandomState(_seed('front', c.shape))
    bn = bn_layer(rs, Ci)
    zf = c.x if x_is_front else rs.randint(-3, 4, (N, H, W, Ci)).astype(np.float32)
    return (zf, bn) + bnred_expected(c.dx, zf, bn, 1.0)
