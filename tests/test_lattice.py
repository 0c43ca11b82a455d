"""CPU proof of what tests/test_exact_conv_gpu.py rests on: for EVERY case of that module the emulated
fp16 split reproduces the digits, every staged half is an fp16 normal number or 0, the exactness condition (per-element sum of
|a| |b| below 2^24 grid units) holds for every output compared, at least a tenth of each operand's non-zero values carry a lo
digit (the generator gives two thirds), and on the smallest case of each operation the expected value equals a brute-force
integer computation."""
import numpy as np
import pytest

import _lattice as lt
import _tileplan as tp
from fractions import Fraction

from oracle import unet_numpy as on


def _pp_n(H, W, Ncols):
    return tp.persistent_family(1, lt.MI355X_CUS, H, W, Ncols)[0]


def _all_cases():
    out = [('conv',) + (k,) + s for k, ss in (('c3', lt.CONV3), ('ct', lt.CONVT)) for s in ss]
    out += [('conv_int',) + s for s in lt.INT_F32]
    out += [('bnin',) + s for s in lt.BNIN]
    out += [('conv', 'c3') + s for s in lt.POOL]
    out += [('bnred',) + s for s in lt.BNRED] + [('conv',) + s for s in lt.BNRED]
    for s in lt.DZIN_DGRAD:
        out += [('dzin', s, dict(with_D=False)), ('dzin', s, dict(with_D=True)), ('dzin', s, dict(with_D=False, two_digit=False))]
    for s in lt.DZIN_WGRAD:
        out += [('dzin', s, dict(with_D=False)), ('dzin', s, dict(with_D=True, bnin=True))]
    out += [('dzin', s, dict(with_D=False, x_int=True)) for s in lt.DZIN_C1]
    out += [('zre',) + s for s in lt.ZRE] + [('stats',) + s for s in lt.STATS] + [('c1stats',) + lt.C1_STATS]
    out += [('guarded',) + s for s in lt.GUARDED]
    for s in lt.JOINT:
        out += [('dzin', s, dict(with_D=False)), ('dzin', s, dict(with_D=True)), ('dzin', s, dict(with_D=False, two_digit=False))]
    out += [('dzin', lt.JOINT[0], dict(with_D=False, bnin=True)), ('dzin', lt.JOINT[0], dict(with_D=False, rank_one=True)),
            ('dzin', lt.JOINT[0], dict(with_D=False, rank_one=True, two_digit=False))]
    for inst, (H, W, Ci, Co) in lt.PP_FWD.items():
        out.append(('conv', 'c3', _pp_n(H, W, Co), H, W, Ci, Co))
    for inst, (H, W, Ci, Co) in lt.PP_DGRAD.items():
        out.append(('conv', 'c3', _pp_n(H, W, Ci), H, W, Ci, Co))
        out.append(('dzin', (_pp_n(H, W, Ci), H, W, Ci, Co), dict(with_D=False)))
    H, W = lt.JOINT_HW
    Nj = tp.persistent_family(1, lt.MI355X_CUS, H, W)[0]
    out += [('dzin', (Nj, H, W, Ci, 32), dict(with_D=False)) for Ci in (32, 64)]
    return out


def _build(case):
    if case[0] == 'conv':
        return lt.conv_case(*case[1:])
    if case[0] == 'conv_int':
        return lt.conv_case(*case[1:], False, 1.0)
    if case[0] == 'bnin':
        return lt.bnin_case(*case[1:])
    if case[0] == 'zre':
        return lt.zre_case(*case[1:])
    if case[0] == 'stats':
        return lt.stats_case(*case[1:])
    if case[0] == 'c1stats':
        return lt.c1_stats_case(*case[1:])
    if case[0] == 'guarded':
        return lt.conv_case(*case[1:], True, lt.GRAD, True)
    if case[0] == 'bnred':
        return lt.bnred_case(*case[1:]).conv
    return lt.dzin_case(*case[1], **case[2])


@pytest.mark.parametrize('case', _all_cases(), ids=lambda c: '-'.join(str(v) for v in c).replace(' ', ''))
def test_case_meets_the_conditions(case):
    """The builders assert the split's exactness, the fp16-normal halves and the 2^24 bound on every expected output; here also
    the digits of every operand under the scale the kernel derives for it, and the lo shares."""
    c = _build(case)
    assert max(c.units.values()) < lt.LIMIT
    if not c.two_digit:
        return
    for name, arr, s, mult in (('x', c.x, getattr(c, 's_x', 1.0), 1.0), ('K', c.K, c.s_k, 1.0),
                               ('dz', c.dz, c.s_dz, getattr(c, 'grad', 1.0))):
        if name not in getattr(c, 'check', ('x', 'K', 'dz')):
            continue
        d1, d0 = lt.digits(arr, mult)
        h, l = lt.halves(arr, s)
        assert np.array_equal(h, d1 * mult) and np.array_equal(l, d0 * lt.G * mult), name      # the split IS the digits
        if name == 'x' and case[0] == 'dzin' and case[2].get('x_int'):
            continue                                     # first layer: fp32 FMA kernels, the image is integer by design
        # two thirds of the generated values carry a lo digit; the ReLU / gate of the on-load cases keeps that share
        assert 0.55 < c.lo[name] < 0.75, (name, c.lo[name])


@pytest.mark.parametrize('s', [1.0, 2.0 ** 9, 2.0 ** 13, 2.0 ** 28, 2.0 ** 11])
def test_split_reproduces_the_digits_under_every_scale(s):
    rs = np.random.RandomState(1)
    mult = lt.GRAD if s == 2.0 ** 28 else 1.0
    v = lt.lattice(rs, (4096,), 0.8, True, mult=mult)
    d1, d0 = lt.digits(v, mult)
    hi, lo = lt.split_f16(v, s)
    assert np.array_equal(hi.astype(np.float64), d1 * mult * s) and np.array_equal(lo.astype(np.float64), d0 * lt.G * mult * s)
    # a value WITHOUT its leading digit goes into hi entirely: the generator never emits one, digits() refuses it
    with pytest.raises(AssertionError):
        lt.digits(np.array([lt.G], np.float32))


def test_scales_restate_the_kernels_rules():
    assert lt.weight_scale(np.array([2.0 + lt.G])) == 2.0 ** 9 and lt.weight_scale(np.array([0.02])) == 2.0 ** 16
    assert lt.guard_scale(np.array([8.0])) == 2.0 ** 11 and lt.guard_scale(None) == 1.0
    assert lt.absmax_scale((2.0 + lt.G) * lt.GRAD) == 2.0 ** 28 and lt.absmax_scale(0.0) == 1.0
    assert lt.absmax_scale(2.0 * lt.GRAD) == 2.0 ** 29


def _units(a, s):
    """(hi, lo) as int64 in units of g / s"""
    h, l = lt.halves(a, s)
    return np.round(h * 4096).astype(np.int64), np.round(l * 4096).astype(np.int64)


@pytest.mark.parametrize('kind', ['c3', 'ct'])
def test_expected_values_equal_integer_arithmetic(kind):
    """Smallest case of each operation: hi and lo as int64 in units of g, the three kept products summed in integers (the
    float64 oracle's loops run on int64 arrays unchanged), against expected3's float64 difference."""
    shape = lt.PREMISE if kind == 'c3' else lt.CONVT[0]
    c = lt.conv_case(kind, *shape)
    fwd, dgrad, wgrad = (lt.op_c3_fwd, lt.op_c3_dgrad, lt.op_c3_wgrad) if kind == 'c3' else (lt.op_ct_fwd, lt.op_ct_dgrad, lt.op_ct_wgrad)
    iz = lambda *s: np.zeros(s, np.int64)
    N, H, W, Ci, Co = shape
    if kind == 'c3':
        ifwd = lambda x, K: on.conv3x3_fwd(x, K, 0)
        idgrad = lambda dz, K: on.conv3x3_bwd(iz(N, H, W, Ci), K, dz)[0]
        iwgrad = lambda x, dz: on.conv3x3_bwd(x, iz(3, 3, Ci, Co), dz)[1]
    else:
        ifwd = lambda x, K: on.convT2x2_fwd(x, K, 0)
        idgrad = lambda dz, K: on.convT2x2_bwd(iz(N, H, W, Ci), K, dz)[0]
        iwgrad = lambda x, dz: on.convT2x2_bwd(x, iz(2, 2, Co, Ci), dz)[1]
    xh, xl = _units(c.x, 1.0)
    kh, kl = _units(c.K, 1.0)
    dh, dl = _units(c.dz / np.float32(c.grad), 1.0)
    U = 4096.0 ** 2
    for op, (ah, al), (bh, bl), want in ((ifwd, (xh, xl), (kh, kl), c.z - lt.f64(c.bias)), (idgrad, (dh, dl), (kh, kl), c.dx / c.grad),
                                         (iwgrad, (xh, xl), (dh, dl), c.dK / c.grad)):
        got = op(ah, bh) + op(ah, bl) + op(al, bh)
        assert got.dtype == np.int64 and np.array_equal(got / U, want)
    if kind == 'c3':       # and element by element in Python ints
        for pix, co in (((0, 0, 0), 0), ((0, 7, 7), 31), ((0, 3, 4), 17)):
            assert lt.brute_c3_fwd_units(c.x, 1.0, c.K, c.s_k, pix, co) == c.z[pix + (co,)] - c.bias[co]


def test_on_load_tables_give_lattice_numbers():
    b = lt.bnin_case('c3', 1, 20, 36, 8, 24)
    assert (b.in_shift > 0).any() and set(np.abs(b.in_scale)) <= {1.0, 2.0} and (b.x == 0).mean() > 0.1
    for with_D in (False, True):
        c = lt.dzin_case(2, 48, 48, 32, 32, with_D)
        assert (c.coef[4] != 0).all() == with_D and np.all(c.coef[6] >= np.abs(c.dz).reshape(-1, 32).max(0))
    r = lt.dzin_case(1, 40, 72, 32, 32, False, rank_one=True)
    assert np.array_equal(r.da, r.s[..., None] * (r.kh[:, 1] - r.kh[:, 0]))


def test_integer_cases_and_sums():
    for s in lt.C1:
        lt.c1_case(*s)
    for s in lt.CONV1D + lt.CONV1D_C1:
        lt.conv1d_case(*s)
    for s in lt.BNRED:
        r = lt.bnred_case(*s)
        assert (r.amax > 0).mean() > 0.5          # a channel whose gate never opens contributes exact zeros
    for s in lt.DZIN_DGRAD + lt.JOINT[:1]:
        c = lt.dzin_case(*s, False, False)
        lt.front_sums(c, x_is_front=s in lt.JOINT)
    # brute force: pass-1 sums of the smallest case in Python ints (units of GRAD / 2)
    r = lt.bnred_case(*lt.BNRED[1])
    c = r.conv
    ch = 5
    gsc = float(r.bn.gamma[ch] * r.bn.invstd[ch])
    gsh = float(r.bn.beta[ch]) - float(r.bn.mean[ch]) * gsc
    s1 = s2 = 0
    for dxv, zv in zip(c.dx[..., ch].ravel(), r.zf[..., ch].ravel()):
        if zv * gsc + gsh > 0:
            d = int(round(dxv / c.grad))
            s1 += 2 * d
            s2 += d * int(round(2 * (float(zv) - float(r.bn.mean[ch])) * float(r.bn.invstd[ch])))
    assert s1 * c.grad / 2 == r.s1[ch] and s2 * c.grad / 2 == r.s2[ch]


def _pick(rs, shape, n=400):
    return [tuple(int(rs.randint(0, d)) for d in shape) for _ in range(n)]


def test_on_load_formations_equal_rational_arithmetic():
    """_bnin, dz from dz_coef (D = 0, D != 0) and the rank-one da, element by element in exact rationals (Python Fractions of
    the fp32 inputs): what the builders form with float64 array expressions is what the table defines."""
    rs = np.random.RandomState(3)
    F = lambda v: Fraction(float(v))
    b = lt.bnin_case('c3', 1, 20, 36, 8, 24)
    for i in _pick(rs, b.x.shape):
        assert max(F(b.z_in[i]) * F(b.in_scale[i[3]]) + F(b.in_shift[i[3]]), 0) == F(b.x[i])
    cases = [lt.dzin_case(2, 48, 48, 32, 32, False), lt.dzin_case(2, 48, 48, 32, 32, True),
             lt.dzin_case(1, 40, 72, 32, 32, False, rank_one=True)]
    for c in cases:
        sc, sh, mu, A, D, E, bound = c.coef
        for i in _pick(rs, c.dz.shape):
            ch = i[3]
            da = F(c.da[i])
            if hasattr(c, 's'):
                da = (F(c.kh[ch, 1]) - F(c.kh[ch, 0])) * F(c.s[i[:3]])
                assert da == F(c.da[i])
            dy = da if F(c.zb[i]) * F(sc[ch]) + F(sh[ch]) > 0 else 0
            dz = F(A[ch]) * dy + (F(D[ch]) * (F(c.zb[i]) - F(mu[ch])) + F(E[ch]))
            assert dz == F(c.dz[i]) and abs(dz) <= F(bound[ch])


def test_conv1d_reference_equals_integer_loops():
    """op_c1d_fwd / op_c1d_wgrad (written for these tests) against plain Python-int loops on the smallest 1-D cases."""
    for shape in (lt.CONV1D[0], lt.CONV1D_C1[0]):
        N, T, Ci, Co = shape
        c = lt.conv1d_case(*shape)
        x, K, dz = (np.round(a).astype(int).tolist() for a in (c.x, c.K, c.dz))
        acc = lt.op_c1d_fwd(lt.f64(c.x), lt.f64(c.K))
        rs = np.random.RandomState(T)
        for n, t, co in _pick(rs, (N, T, Co), 200) + [(0, 0, 0), (N - 1, T - 1, Co - 1), (0, 1, 0), (0, T - 2, 1)]:
            v = sum(x[n][t + k - 2][ci] * K[k][ci][co] for k in range(5) if 0 <= t + k - 2 < T for ci in range(Ci))
            assert v == acc[n, t, co]
            assert max(Fraction(v) * Fraction(float(c.scale[co])) + Fraction(float(c.shift[co])), 0) == Fraction(c.y[n, t, co])
        for k, ci, co in _pick(rs, (5, Ci, Co), 60) + [(0, 0, 0), (4, Ci - 1, Co - 1)]:
            v = sum(x[n][t + k - 2][ci] * dz[n][t][co] for n in range(N) for t in range(T) if 0 <= t + k - 2 < T)
            assert v == c.dK[k, ci, co]


def test_stats_and_rebuilt_z_cases():
    for s in lt.STATS:
        c = lt.stats_case(*s)
        assert c.sums.shape == (s[5], 2) and np.array_equal(c.sums, np.round(c.sums))
    c = lt.c1_stats_case(*lt.C1_STATS)
    assert np.array_equal(c.sums, np.round(c.sums))
    r = lt.zre_case(*lt.ZRE[0])
    # brute force: one kernel-gradient element of the rebuilt-z case in exact rationals
    N, H, W, _, Co = r.shape
    co, tap = 3, (0, 2)
    tot = Fraction(0)
    for n in range(N):
        for y in range(H):
            for xx in range(W):
                zz = Fraction(float(r.bias[co]))
                for a in range(3):
                    for b in range(3):
                        if 0 <= y + a - 1 < H and 0 <= xx + b - 1 < W:
                            zz += Fraction(float(r.x[n, y + a - 1, xx + b - 1, 0])) * Fraction(float(r.w[a, b, 0, co]))
                gate = zz * Fraction(float(r.coef[0, co])) + Fraction(float(r.coef[1, co])) > 0
                dz = Fraction(float(r.coef[3, co])) * (Fraction(float(r.da[n, y, xx, co])) if gate else 0)
                yy, xs = y + tap[0] - 1, xx + tap[1] - 1
                if 0 <= yy < H and 0 <= xs < W:
                    tot += Fraction(float(r.x[n, yy, xs, 0])) * dz
    assert tot == Fraction(float(r.dK[tap[0], tap[1], 0, co]))
