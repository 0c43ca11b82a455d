"""CPU checks of tests/_tileplan.py: the mirror reproduces the hand-replayed launch plans, and every row of the case
tables of tests/test_multitile_gpu.py and tests/test_spikes_multitile_gpu.py really has the tiles per workgroup, the
short last split and the ragged edges it claims -- a later change of shapes cannot quietly fall back to one tile per workgroup."""
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


# ---- UNet1D (tests/test_spikes_multitile_gpu.py) ---------------------------------------------------------------------------
WGRAD1D_INSTANTIATIONS = ['32x32', '64x32', '32x64', '64x64']


def _crosses_a_trace(per_trace, total, tps, splits):
    return any((s * tps) // per_trace != (min(total, (s + 1) * tps) - 1) // per_trace for s in range(splits))


def test_wgrad1d_mirror_reproduces_the_hand_replayed_plans():
    # production (batch 20, 4096 frames, nfb 32) -> tiles_total, tiles_per_split, splits, last_split_tiles
    for shape, exp in [((20, 4096, 32, 32), (640, 2, 320, 2)),
                       ((20, 4096, 96, 32), (1280, 5, 256, 5)),
                       ((20, 512, 768, 256), (160, 15, 11, 10))]:
        assert tp.wgrad1d_plan(*shape)[5:] == exp, (shape, tp.wgrad1d_plan(*shape))
    # tile width and (m, n) block of every instantiation, at the thresholds of the dispatch
    assert tp.wgrad1d_plan(1, 64, 36, 36)[:4] == ('64x64', 64, 64, 64)
    assert tp.wgrad1d_plan(1, 64, 36, 32)[:4] == ('64x32', 64, 64, 32)
    assert tp.wgrad1d_plan(1, 64, 32, 36)[:4] == ('32x64', 64, 32, 64)
    assert tp.wgrad1d_plan(1, 64, 32, 32)[:4] == ('32x32', 128, 32, 32)
    # the gap the multi-tile module closes: every shape of the direct tests runs ONE tile per workgroup, at most 12 slabs
    for shape in tp.WGRAD1D_DIRECT_SHAPES:
        plan = tp.wgrad1d_plan(*shape)
        assert plan[6] == 1 and plan[7] == plan[5] <= 12, (shape, plan)
    assert tp.wgrad1d_plan(6, 200, 4, 4)[5:] == (12, 1, 12, 1)       # "more than one contraction partition": 12 tiles, 12 workgroups


@pytest.mark.parametrize('case', tp.WGRAD1D_CASES, ids=lambda c: '%s-%dx%dx%dx%d' % c[:5])
def test_wgrad1d_case_has_the_claimed_plan(case):
    inst, N, T, Cin, Cout, tps, last = case
    got_inst, TW, CM, CN, per_trace, total, got_tps, splits, got_last = tp.wgrad1d_plan(N, T, Cin, Cout)
    assert got_inst == inst and (got_tps, got_last) == (tps, last)
    assert tps >= 2 and 1 <= last <= tps and (splits - 1) * tps + last == total and splits > 1
    assert T % TW != 0                                           # the last tile of every trace is ragged
    assert per_trace == tp.cdiv(T, TW) and total == N * per_trace
    assert _crosses_a_trace(per_trace, total, tps, splits)
    if per_trace > 1:                                            # ranges start and end in the middle of a trace
        assert per_trace % tps != 0 and tps % per_trace != 0
    assert 4 * N * T * (Cin + Cout) <= 13.5e6                    # the operand pair stays small
    # the library's own size guard (wgrad1d_shape_ok) holds by a wide margin
    assert T * max(Cin, Cout) < 2 ** 31 and 5 * Cin * Cout < 2 ** 31


def test_wgrad1d_table_covers_every_instantiation():
    assert sorted({c[0] for c in tp.WGRAD1D_CASES}) == sorted(WGRAD1D_INSTANTIATIONS)
    ragged_both = 0
    for inst in WGRAD1D_INSTANTIATIONS:
        rows = [c for c in tp.WGRAD1D_CASES if c[0] == inst]
        assert any(c[5] == 2 and c[6] == 1 for c in rows), (inst, '2 tiles, last split 1')
        assert any(c[5] == 3 for c in rows), (inst, 3)
        assert any(c[5] >= 5 for c in rows), (inst, 'at least 5')
        assert any(c[2] == 5 for c in rows) and any(tp.wgrad1d_plan(*c[1:5])[4] > 1 for c in rows), (inst, 'both kinds of rows')
        # dc_reduce_partials' two-stage path (64 slabs or more) through every instantiation
        assert any(tp.wgrad1d_plan(*c[1:5])[7] >= 64 for c in rows), (inst, 'no row with 64 slabs')
        for c in rows:
            _, _, CM, CN = tp.wgrad1d_plan(*c[1:5])[:4]
            ragged_both += c[3] % CM != 0 and c[4] % CN != 0
    assert ragged_both >= 2
    assert ('64x64', 7, 450, 768, 256, 6, 2) in tp.WGRAD1D_CASES           # the widest contraction of the real network


def test_wgrad1d_probe_rows():
    assert [c[0] for c in tp.WGRAD1D_PROBE_CASES] == WGRAD1D_INSTANTIATIONS
    for inst, N, T, Cin, Cout, tps, last in tp.WGRAD1D_PROBE_CASES:
        per_trace = tp.wgrad1d_plan(N, T, Cin, Cout)[4]
        assert per_trace > 1 and last < tps and N >= 8


def test_conv1d_fwd_grids_and_reduction_caps():
    for (N, T, Cin, Cout), grid in tp.CONV1D_FWD_CASES:
        assert tp.conv1d_fwd_grid(N, T, Cout) == grid == N * tp.cdiv(T, 128) * tp.cdiv(Cout, 64)
    grids = [g for _, g in tp.CONV1D_FWD_CASES]
    assert sorted(g % 8 for g in grids if g > 8) == [0, 0, 3, 4, 4] and sum(g <= 8 for g in grids) == 1
    # the direct tests (CONV_SHAPES of test_spikes_gpu.py, GRAD_SHAPES as data gradients) stay at 8 workgroups or fewer
    for N, T, Cin, Cout in [(1, 1, 4, 4), (2, 3, 8, 4), (3, 37, 12, 36), (2, 130, 32, 32), (2, 70, 768, 256), (1, 260, 8, 72)]:
        assert tp.conv1d_fwd_grid(N, T, Cout) <= 8
    for N, T, Cin, Cout in tp.WGRAD1D_DIRECT_SHAPES[:5]:
        assert tp.conv1d_fwd_grid(N, T, Cin) <= 8
    # the two vector reductions: the direct tests stay below their caps, the multi-tile module's shapes pass them
    for N, T, C in [(1, 1, 4), (3, 37, 12), (2, 300, 32)]:                   # test_conv1d_stats
        blocks, trips = tp.quad_plan(N * T, C, 16, 1024)
        assert blocks < 1024 and trips <= 16
    for N, T, C in [(1, 16, 4), (3, 37, 32), (2, 2100, 8)]:                  # test_conv1d_k5_c1_wgrad
        blocks, trips = tp.quad_plan(N * T, C, 32, 512)
        assert blocks < 512 and trips <= 32
    assert tp.quad_plan(16384 + 37, 1024, 16, 1024) == (1024, 17)
    assert tp.quad_plan(3 * 5477, 1024, 32, 512) == (512, 33)


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
