"""CPU checks of tests/_gridcaps.py, which tests/test_grid_caps_gpu.py builds on: the f % K bookkeeping of the periodic recordings,
the two vectorised oracles against the plain ones, and the arithmetic by which every shape of the GPU module crosses its cap -- a
later change of a shape cannot quietly fall back to one trip per workgroup."""
import numpy as np

import _dff_ref as dref
import _gridcaps as gc

LIM = 2 ** 62 - 1


def test_periodic_recordings_name_the_right_base_frame():
    rs = np.random.RandomState(0)
    for dtype in (np.int16, np.uint16):
        base = gc.base_frames(rs, (3, 5), dtype)
        info = np.iinfo(dtype)
        assert base.dtype == dtype and base.min() == info.min and base.max() == info.max
        n = gc.THREE_TRIPS
        rec = gc.expand(base, n)
        assert rec.shape == (n, 3, 5) and rec.dtype == dtype
        for f in (0, 1, gc.K - 1, gc.K, gc.FRAME_CAP - 1, gc.FRAME_CAP, gc.FRAME_CAP + 1, 2 * gc.FRAME_CAP, n - 1):
            assert np.array_equal(rec[f], base[f % gc.K]) and gc.rows(n)[f] == f % gc.K
    tables = rs.randint(-9, 9, size=(gc.K, 2))
    assert np.array_equal(gc.expand(tables, 100)[77], tables[77 % gc.K])
    # a kernel that takes the frame one stride early (or late) on a later trip meets another base frame: K divides no stride
    for stride in (gc.FRAME_CAP, gc.ITEM_CAP // 16, gc.FRAME_CAP * gc.TRACE_TILE, gc.ZERO_CAP):
        assert stride % gc.K != 0
        f = np.arange(stride, stride + 500)
        assert (gc.rows(stride + 500)[f] != gc.rows(stride + 500)[f - stride]).all()


def test_every_shape_crosses_its_cap():
    assert gc.FRAME_CAP < gc.TWO_TRIPS <= 2 * gc.FRAME_CAP < gc.THREE_TRIPS <= 3 * gc.FRAME_CAP
    assert gc.first_stride_trip(gc.TWO_TRIPS, gc.FRAME_CAP) == gc.FRAME_CAP and gc.first_stride_trip(37, gc.FRAME_CAP) is None
    # the zero kernels: the smallest score table of the module, and the two sums of the trace module, are more than one trip
    assert gc.THREE_TRIPS * 9 > gc.ZERO_CAP and gc.TWO_TRIPS * 9 > gc.ZERO_CAP and 2 * gc.TRACE_FRAMES > gc.ZERO_CAP
    # dc_motion_block_pick: 4 x 4 blocks of TWO_TRIPS frames are more items than workgroups, the rest lie in the last frames
    items = gc.TWO_TRIPS * 16
    assert items == 1049216 > gc.ITEM_CAP and gc.ITEM_CAP // 16 == 65536
    # dc_roi_trace_accumulate, dc_trace_*: tiles beyond 65535
    assert -(-gc.TRACE_FRAMES // gc.TRACE_TILE) == gc.FRAME_CAP + 3 and gc.TRACE_FRAMES % gc.TRACE_TILE == 6
    assert -(-gc.DFF_FRAMES // gc.DFF_TILE) == gc.FRAME_CAP + 2 and gc.DFF_FRAMES % gc.DFF_TILE == 44
    # dc_motion_apply: the big frame has more groups of 8 than 4096 * 256 threads; every second-trip group lies in the band
    H, W = gc.BIG_H, gc.BIG_W
    assert H * W == 8407049 > 8 * gc.APPLY_X_CAP * 256
    assert (H * W) % 8 == 1                               # the second frame starts one value off a group: its groups straddle rows
    assert gc.apply_second_trip_rows(H, W, 2) == (2046, H - 1) and 2046 >= H - gc.BIG_BAND
    assert gc.apply_second_trip_rows(16, 64, 33) is None and gc.apply_second_trip_rows(40, 1100, 2) is None     # the existing shapes
    # the small movers: H W odd, so the frames' first values walk through every residue of 8
    assert {(t * 15) & 7 for t in range(8)} == set(range(8)) and {(t * 55) & 7 for t in range(8)} == set(range(8))


def test_vectorised_baseline_is_the_sorted_window():
    rs = np.random.RandomState(1)
    x = rs.randint(-1000, 1001, size=(2, 1000)).astype(np.int64)
    x[0, 100:140] = 7                                     # ties
    x[1, [0, 1, 500, 501, 998, 999]] = [LIM, -LIM, -LIM, LIM, LIM, -LIM]
    for q in (0, 8, 49, 50, 51, 99, 100):
        assert np.array_equal(gc.baseline_half1(x, q), dref.baseline(x, 1, q)), q
    for T in (1, 2, 3):
        for q in (0, 50, 100):
            assert np.array_equal(gc.baseline_half1(x[:, :T], q), dref.baseline(x[:, :T], 1, q)), (T, q)


def test_vectorised_roi_sums():
    rs = np.random.RandomState(2)
    for dtype in (np.int16, np.uint16):
        frames = gc.base_frames(rs, (2, 3), dtype)
        pixels = [[0, 1, 5], [2, 3, 4], [4]]
        got = gc.roi_sums(frames, pixels)
        assert got.dtype == np.int64 and got.shape == (3, gc.K)
        for r, p in enumerate(pixels):
            for t in range(gc.K):
                assert got[r, t] == sum(int(frames[t].flat[i]) for i in p)
