"""CPU checks of tests/_ewcaps.py, which tests/test_ew_caps_gpu.py builds on: the caps are the ones csrc/elementwise.hip states,
every shape of the GPU module lands in the regime its test claims -- a later change of a shape or of a cap cannot quietly fall back
to one trip per thread --, and the numpy oracle of dc_crop_augment is the dihedral table of the package."""
import os
import re

import numpy as np

import _ewcaps as ec

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'deep_calcium_amd', 'csrc', 'elementwise.hip')


def _body(src, name):
    """The text of the entry point (or helper) `name`, up to the closing brace in column 0."""
    m = re.search(r'^(?:extern "C" |static )int %s\(.*?^}' % re.escape(name), src, flags=re.M | re.S)
    assert m, name
    return m.group(0)


def test_the_caps_are_the_ones_the_source_states():
    src = open(SRC).read()
    assert re.search(r'static const int kMaxBlocks = %d;' % ec.K_MAX_BLOCKS, src)
    assert 'static const int kMaxBwdBlocks = kMaxBlocks;' in src
    assert 'const int PPB = 256 / (C / 4);' in _body(src, 'ew_blocks') and ec.ppb(32) == 32 and ec.ppb(4) == 256 and ec.ppb(1024) == 1
    for name, cap in (('dc_maxpool2x2_fwd', ec.CAP_4096), ('dc_maxpool2x2_bwd', ec.CAP_4096), ('pool_bwd_blocks', ec.CAP_2048),
                      ('dc_upsample2x_drop_fwd', ec.CAP_4096), ('dc_upsample2x_drop_bwd', ec.CAP_4096),
                      ('dc_adam_step_flat', ec.CAP_4096), ('dc_fill', ec.CAP_2048), ('dc_scale_flat', ec.CAP_2048),
                      ('dc_gather_maps', ec.CAP_4096), ('dc_tta_merge', ec.CAP_4096), ('dc_crop_augment', ec.CROP_CAP),
                      ('dc_round_window_u8', ec.ROUND_CAP), ('head_blocks', ec.HEAD_CAP)):
        assert re.search(r'\+ 255\) / 256 > %d \? %d :|b > %d \? %d :' % (cap, cap, cap, cap), _body(src, name)), (name, cap)
    assert 'blocks > kMaxBlocks' in _body(src, 'dc_bn_relu_drop_pool_fwd')
    for name in ('dc_bn_relu_drop_fwd', 'dc_bn_bwd_reduce', 'bn_bwd_apply_impl'):
        assert re.search(r'dim3\(ew_(bwd_)?blocks\(pixels, C\)\)', _body(src, name)), name
    assert 'dim3(pool_bwd_blocks(N, H, W, C))' in _body(src, 'dc_maxpool2x2_bwd_bnred')


def test_trip_helpers():
    assert ec.lane_trips(10, 4) == (3, 2) and ec.lane_trips(8, 4) == (2, 2) and ec.lane_trips(3, 4) == (1, 0)
    assert ec.flat_trips(256 * 4096, 4096) == (1, 1) and ec.flat_trips(256 * 4096 + 1, 4096) == (2, 1)
    assert ec.flat_trips(1024, 4096) == (1, 1) and ec.flat_blocks(1000, 4096) == 4 and ec.flat_trips(1000, 4096) == (1, 0)
    assert ec.bn_blocks(1, 32) == 1 and ec.bn_blocks(33, 32) == 2 and ec.bn_blocks(10 ** 7, 32) == 1280
    for C in (4, 8, 32, 256, 1024):
        assert ec.bn_stride(C) * C == 1280 * 1024
    assert ec.sweep_census(5, 1024) == {(0, 1): 5}
    # the shapes the older modules reach: every lane owns one pixel at most, the two-pixel body never runs ...
    for shape, C in (((2, 16, 16), 32), ((1, 24, 40), 8), ((3, 8, 8), 256), ((4, 6, 10), 64)):
        px = shape[0] * shape[1] * shape[2]
        assert ec.bn_blocks(px, C) < ec.K_MAX_BLOCKS and set(ec.sweep_census(px, C)) <= {(0, 1), (0, 0)}
    # ... but for the self-comparison of tests/test_dropout_rng_gpu.py
    assert set(ec.sweep_census(4 * 40 * 44, 256)) == {(1, 0), (0, 1)}


def test_bn_shapes_land_in_their_regimes():
    seen = {}
    for regime, C, drop, ld in ec.BN_CASES:
        P, s = ec.bn_pixels(regime, C), ec.bn_stride(C)
        assert ec.bn_blocks(P, C) == ec.K_MAX_BLOCKS and ld >= C and ld % 4 == 0
        assert ec.sweep_trips(P, C) == ec.BN_REGIMES[regime][0], (regime, C)
        assert ec.bn_trips(P, C)[0] >= 2                                  # the forward: a second trip at least
        assert P * C <= 3.5 * 1280 * 1024 + 3 * C                         # 4.6 M floats per tensor at most
        seen.setdefault(regime, set()).add(C)
        seen.setdefault(drop, set()).add(C)
        census = ec.sweep_census(P, C)
        assert sum(census.values()) == s and sum((2 * b + t) * n for (b, t), n in census.items()) == P
        if regime == 0:
            assert census == {(1, 0): 1, (0, 1): s - 1}
        elif regime == 1:
            assert census == {(1, 0): s // 2 + 3, (0, 1): s - s // 2 - 3}
        elif regime == 2:
            assert census == {(1, 0): s}
        elif regime == 3:
            assert census == {(1, 1): 1, (1, 0): s - 1}
        elif regime == 4:
            assert census == {(1, 1): s // 2 + 3, (1, 0): s - s // 2 - 3}
        else:
            assert census == {(2, 0): s // 2 + 3, (1, 1): s - s // 2 - 3}
    for regime in range(6):
        assert 32 in seen[regime] and len(seen[regime]) >= 2, regime
    for drop in ('none', 'mask', 'rng'):
        assert seen[drop] == {4, 32, 1024}, drop
    assert any(ld > C for _, C, _, ld in ec.BN_CASES) and any(ld == C for _, C, _, ld in ec.BN_CASES)


def test_flat_shapes_cross_their_caps():
    one = ec.K_MAX_BLOCKS * ec.THREADS
    assert one == 327680
    trips = [ec.lane_trips(ec.pool_items(*sh), one) for sh in ec.POOL_FUSED_SHAPES]
    assert trips == [(2, 1), (3, 2), (2, 1)] and [sh[3] for sh in ec.POOL_FUSED_SHAPES] == [32, 32, 4]
    assert all(ec.pool_items(*sh) > one for sh in ec.POOL_FUSED_SHAPES)
    items = ec.pool_items(*ec.POOL_SHAPE)
    assert items == 1365174 and 1.25 < items / (ec.CAP_4096 * ec.THREADS) < 1.35 and items % ec.THREADS == 182      # ragged
    assert ec.flat_trips(items, ec.CAP_4096) == (2, 1)
    for sh in ec.POOL_BNRED_SHAPES:
        items = ec.pool_items(*sh)
        assert items == 1081600 and ec.flat_blocks(items, ec.CAP_2048) == ec.CAP_2048 and ec.flat_trips(items, ec.CAP_2048) == (3, 2)
        assert (ec.CAP_2048 * ec.THREADS) % (sh[3] // 4) == 0         # the stride keeps a thread's channel quad
    assert [sh[3] // 4 for sh in ec.POOL_BNRED_SHAPES] == [2, 64]
    for n, rem in zip(ec.ADAM_N, (2, 3)):
        assert n % 4 == rem and ec.flat_trips(n // 4, ec.CAP_4096) == (3, 2) and ec.flat_blocks((n + 3) // 4, ec.CAP_4096) == 4096
        assert 2 * ec.ADAM_TRIP < n - n % 4 < 3 * ec.ADAM_TRIP
    assert ec.FILL_N == 524365 and ec.flat_trips(ec.FILL_N, ec.CAP_2048) == (2, 1)
    t = ec.TTA
    assert t['hs'] * t['ws'] == 1058837 > ec.CAP_4096 * ec.THREADS and ec.flat_trips(t['hs'] * t['ws'], ec.CAP_4096) == (2, 1)
    assert t['hs'] < t['H'] and t['ws'] < t['W']
    # dc_crop_augment: 64 x 256 threads per image; the existing tests stop at hw = 64
    assert ec.crop_threads(64) <= ec.CROP_CAP * ec.THREADS and ec.crop_threads(256) == ec.CROP_CAP * ec.THREADS
    assert [ec.lane_trips(ec.crop_threads(hw), ec.CROP_CAP * ec.THREADS) for hw in ec.CROP_HW] == [(2, 1), (4, 4)]
    assert ec.crop_threads(260) - ec.CROP_CAP * ec.THREADS == 516         # the ragged second trip
    r = ec.ROUND
    per = (r['y1'] - r['y0']) * (r['x1'] - r['x0'])
    assert (r['y1'] - r['y0'], r['x1'] - r['x0']) == (258, 255) and per == 65790
    assert ec.lane_trips(per, ec.ROUND_CAP * ec.THREADS) == (2, 1) and 1363 < ec.ROUND_CAP * ec.THREADS
    assert r['y1'] < r['H'] and r['x1'] < r['W'] and r['y0'] > 0 and r['x0'] > 0


def test_crop_oracle_is_the_packages_dihedral_table():
    from deep_calcium_amd import unet2ds
    a = np.arange(35 * 35).reshape(35, 35)
    maps = [ec.d4_apply(a, d4) for d4 in range(8)]
    assert len({m.tobytes() for m in maps}) == 8
    for d4 in range(8):
        assert unet2ds._d4_bits(lambda x, d4=d4: ec.d4_apply(x, d4)) == d4
        i, j = 3, 10                                          # the header's formula at one pixel
        r, c = (j, i) if d4 & 1 else (i, j)
        r = 34 - r if d4 & 2 else r
        c = 34 - c if d4 & 4 else c
        assert maps[d4][i, j] == a[r, c]
    numpy_table = [a, np.fliplr(a), np.flipud(a), np.rot90(a, 1), np.rot90(a, 2), np.rot90(a, 3), np.rot90(a, 1)[:, ::-1], np.rot90(a, 1)[::-1]]
    assert {m.tobytes() for m in maps} == {np.ascontiguousarray(m).tobytes() for m in numpy_table}
    S = np.arange(1, 1 + 50 * 60, dtype=np.float32).reshape(50, 60)
    w = ec.crop_ref(S, 4, 7, 5, 3, 8, 0)
    assert w.shape == (8, 8) and np.array_equal(w[:5, :3], S[4:9, 7:10]) and w[5:].sum() == 0 and w[:, 3:].sum() == 0
    assert np.array_equal(ec.crop_ref(S, 4, 7, 5, 3, 8, 6), w[::-1, ::-1])
    items = ec.crop_items(16, (50, 60), np.random.RandomState(0))
    assert sorted(it[4] for it in items) == sorted(list(range(8)) * 2) and sum(it[2] < 16 or it[3] < 16 for it in items) == 8
