"""CPU checks of tests/_tileplan.py: the mirror reproduces the hand-replayed launch plans, and every row of the case
tables of tests/test_multitile_gpu.py really has the tiles per workgroup, the short last split and the ragged edges it
claims -- a later change of shapes cannot quietly fall back to one tile per workgroup."""
import pytest

import _tileplan as tp

ALL_WGRAD = tp.WGRAD_CASES + tp.CONVT_WGRAD_CASES
INSTANTIATIONS = {'conv': ['W<=8', 'W<=16', '64x64', '64x32', '32x64', '32x32'], 'convT': ['W<=8', 'Cin>=128', 'rest']}


def test_mirror_reproduces_the_hand_replayed_plans():
    # (kind, N, H, W, Cin, Cout) -> tiles_total, tiles_per_split, splits, last_split_tiles (None: not established by hand)
    for shape, exp in [(('conv', 2, 40, 40, 144, 96), (60, 2, None, None)),
                       (('conv', 20, 16, 16, 256, 256), (80, 5, None, None)),
                       (('conv', 20, 8, 8, 512, 512), (20, 5, 4, 5)),
                       (('conv', 16, 512, 512, 32, 32), (16384, 64, 256, 64)),
                       (('conv', 7, 12, 12, 256, 256), (21, 2, 11, 1)),
                       (('convT', 5, 6, 6, 512, 256), (5, 2, 3, 1)),
                       (('conv', 2, 27, 24, 256, 256), (28, 2, 14, 2))]:
        got = tp.wgrad_plan(*shape)[4:]
        for g, e in zip(got, exp):
            assert e is None or g == e, (shape, got, exp)
    # the existing direct tests' shapes with one tile per workgroup stay what they are
    assert tp.wgrad_plan('conv', 2, 64, 64, 64, 64)[5] == 1 and tp.wgrad_plan('convT', 2, 32, 32, 64, 32)[5] == 1
    # tile shapes and (m, n) blocks of every instantiation
    assert tp.wgrad_plan('conv', 1, 8, 8, 64, 64)[:4] == (8, 8, 64, 64)
    assert tp.wgrad_plan('conv', 1, 16, 16, 64, 64)[:4] == (16, 4, 64, 64)
    assert tp.wgrad_plan('conv', 1, 64, 64, 64, 64)[:4] == (16, 4, 64, 64)
    assert tp.wgrad_plan('conv', 1, 64, 64, 64, 32)[:4] == (32, 4, 64, 32)
    assert tp.wgrad_plan('conv', 1, 64, 64, 32, 64)[:4] == (32, 4, 32, 64)
    assert tp.wgrad_plan('conv', 1, 64, 64, 32, 32)[:4] == (32, 8, 32, 32)
    assert tp.wgrad_plan('convT', 1, 8, 8, 64, 64)[:4] == (8, 8, 32, 64)
    assert tp.wgrad_plan('convT', 1, 32, 32, 128, 64)[:4] == (16, 4, 32, 128)
    assert tp.wgrad_plan('convT', 1, 32, 32, 64, 64)[:4] == (16, 4, 32, 64)


@pytest.mark.parametrize('case', ALL_WGRAD, ids=lambda c: '%s-%s-%dt' % (c[0], c[1], c[7]))
def test_weight_gradient_case_has_the_claimed_plan(case):
    kind, inst, N, H, W, Cin, Cout, tps, last = case
    assert tp.wgrad_instantiation(kind, W, Cin, Cout) == inst
    TW, TH, CM, CN, total, got_tps, splits, got_last = tp.wgrad_plan(kind, N, H, W, Cin, Cout)
    assert (got_tps, got_last) == (tps, last)
    assert 1 <= last <= tps and (splits - 1) * tps + last == total and splits > 1
    assert N >= 2
    if inst.startswith('W<='):          # a tile is an image column: ragged = the image is smaller than the tile
        assert W < TW or H < TH
    else:
        assert H % TH != 0 or W % TW != 0
    # some workgroup's tile range crosses an image boundary
    per_img = total // N
    assert any((s * tps) // per_img != (min(total, (s + 1) * tps) - 1) // per_img for s in range(splits))


def test_weight_gradient_table_covers_every_instantiation_at_2_3_4_5_tiles():
    for kind, names in INSTANTIATIONS.items():
        for inst in names:
            rows = [c for c in ALL_WGRAD if c[0] == kind and c[1] == inst]
            assert any(c[7] == 2 and c[8] == 1 for c in rows), (kind, inst, '2 tiles, last split 1')
            assert any(c[7] == 3 for c in rows), (kind, inst, 3)
            assert any(c[7] == 4 and c[8] < 4 for c in rows), (kind, inst, '4 tiles, short last split')
            assert any(c[7] == 5 for c in rows), (kind, inst, 5)
            ragged_ch = False
            for c in rows:
                _, _, CM, CN = tp.wgrad_plan(*((c[0],) + c[2:7]))[:4]
                Cm, Cn = (c[5], c[6]) if kind == 'conv' else (c[6], c[5])
                ragged_ch |= Cm % CM != 0 or Cn % CN != 0
            assert ragged_ch, (kind, inst, 'no channel count that is not a multiple of the block')


@pytest.mark.parametrize('case', tp.C1_WGRAD_CASES)
def test_first_layer_case_runs_its_loop_more_than_once(case):
    N, H, W, Cout, trips = case
    assert tp.c1_plan(N, H, W, Cout) == (2048, trips) and trips > 1
    assert tp.c1_plan(2, 64, 64, 16)[1] == 1          # the existing direct test's largest shape: one trip
    assert [c[2] % 4 == 0 for c in tp.C1_WGRAD_CASES] == [True, False]      # both kernels


def test_persistent_plan_distribution():
    # every item exactly once, n or n + 1 per workgroup, whatever the remainders
    for items, cus in [(260, 256), (276, 256), (780, 256), (516, 256), (308, 304), (100, 256), (1024, 256), (257, 256), (2047, 256)]:
        plan = tp.persistent_plan(items, cus)
        assert len(plan) == min(items, cus)
        assert sorted(i for wg in plan for i in wg) == list(range(items))
        lens = {len(wg) for wg in plan}
        assert max(lens) - min(lens) <= 1 or items % 8 != 0
        if items % 8 == 0 and items % cus == 0:
            assert lens == {items // cus}
    # the even, power-of-two launches of the existing tests: no workgroup differs from its neighbour
    assert {len(wg) for wg in tp.persistent_plan(1024, 256)} == {4}
    # the family the GPU module derives: k and k + 1 items side by side, uneven over the XCDs
    for cus in (256, 304, 64):
        for k, H, W, Ncols in [(1, 12, 40, 160), (3, 12, 40, 160), (3, 12, 40, 64), (1, 20, 40, 32), (3, 20, 40, 32), (1, 10, 40, None),
                               (2, 10, 40, None)]:
            found = tp.persistent_family(k, cus, H, W, Ncols)
            assert found is not None, (cus, k, H, W, Ncols)
            N, items = found
            assert N >= 2 and k * cus < items < (k + 1) * cus and items % 8 != 0
            assert items == (tp.pp_items(N, H, W, Ncols) if Ncols else tp.joint_items(N, H, W))
            assert {len(wg) for wg in tp.persistent_plan(items, cus)} == {k, k + 1}


def test_item_counts():
    assert tp.pp_items(8, 128, 128, 128) == 1024 and tp.pp_items(16, 128, 128, 64) == 1024      # the existing tests' even launches
    assert tp.pp_tile(32) == (16, 32, 32) and tp.pp_tile(33) == (8, 32, 64)
    assert tp.pp_items(1, 20, 40, 32) == 4 and tp.pp_items(1, 12, 40, 160) == 12 and tp.pp_tiles(1, 12, 40, 160) == 4
    assert tp.joint_items(16, 32, 32) == 128 and tp.joint_items(3, 33, 50) == 54
