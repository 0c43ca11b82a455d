"""CPU checks of tests/_wideindex.py, which tests/test_wide_index_gpu.py builds on: the arithmetic by which every shape crosses the
32-bit line (or its grid cap) at the smallest size, where a kernel that keeps 31 bits of an offset lands -- inside the allocation,
on other valid data --, the table against a census of the header, the memory budget, and the census of the entry points that
DC_FRAMES_PER_CALL_MAX bounds.  A later change of a shape cannot quietly fall back below the line."""
import ctypes
import os
import re

import numpy as np

import _gridcaps as gc
import _wideindex as wi
from deep_calcium_amd import _lib

I32_MAX = 2 ** 31 - 1
HERE = os.path.dirname(os.path.abspath(__file__))


def test_row_cases_cross_the_line_and_the_masked_offset_stays_inside():
    assert wi.LINE == I32_MAX + 1 and wi.MASK == I32_MAX
    R, ld, T = wi.ROW_A
    assert R == 2 and ld == 2 ** 31 + 8 > I32_MAX and T == 300                       # A: ld itself is beyond int32
    R, ld, T = wi.ROW_B
    assert R == 3 and ld == 2 ** 30 + 5 <= I32_MAX and (R - 1) * ld == 2 ** 31 + 10   # B: each factor fits, the product does not
    assert wi.ROW_B65 == (3, 2 ** 30 + 5, 65)                                        # one frame past the 64-frame tile of the forward walk
    assert 300 == 256 + 44                                                           # a full tile of 256 frames and a ragged one
    for name, want in (('A', 8), ('B', 10), ('B65', 10)):
        case = wi.ROW_CASES[name]
        R, ld, T = case
        first = wi.last_row_offset(case)
        assert first > I32_MAX and (first - ld <= I32_MAX or R == 2)                 # the last row is the only one beyond the line
        n = wi.row_elements(case)
        assert n == (R - 1) * ld + T < R * ld                                        # the last row carries no padding
        off = wi.decoy_offset(case)
        assert off == first & 0x7fffffff == want
        # a kernel that keeps 31 bits of the offset reads (or writes) [off, off + T): inside the buffer, over the tail of row 0 and the
        # `off` planted values behind it, short of row 1
        assert 0 < off and off + T <= T + off < ld and off + T < n
        # ... and so does one that keeps 32 bits: the offsets here are below 2^32, it is right
        assert first < 2 ** 32
    assert wi.row_elements(wi.ROW_A) * 4 // wi.GiB == 8 and wi.row_elements(wi.ROW_A) * 8 // wi.GiB == 16
    assert wi.row_elements(wi.ROW_B) * 8 // wi.GiB == 16


def test_frame_route_crosses_the_line_on_a_third_trip_and_aliases_another_base_frame():
    H, W = wi.FRAME_HW
    hw, tc = H * W, wi.FRAME_TC
    assert (H, W) == (128, 128) and tc == 131113
    assert tc * hw == 2148155392 and tc * hw * 2 / wi.GiB > 4.0
    first = -(-wi.LINE // hw)
    assert first == 131072 and wi.frame_offset(first) == wi.LINE and wi.frame_offset(first - 1) <= I32_MAX
    assert 2 * gc.FRAME_CAP < first < tc <= 3 * gc.FRAME_CAP                          # the frames beyond the line: a third trip of the grid
    assert first % gc.K == 18 and wi.K == gc.K == 37
    f = np.arange(first, tc)
    alias = np.array([wi.aliased_frame(int(v)) for v in f])
    assert np.array_equal(alias, f - first) and (alias < first).all()               # inside the recording
    assert (f % gc.K != alias % gc.K).all()                                          # and another base frame: a different answer
    # the sums over all frames differ as well: the 41 aliased frames are not the same multiset of base frames
    assert sorted((f % gc.K).tolist()) != sorted((alias % gc.K).tolist())
    # a mover's `out` from frame 131072 on, 3 values into its allocation: the same frames, never on a group of 8
    assert all((3 + int(v) * hw) % 8 == 3 for v in (0, 1, first, tc - 1))
    # dc_frame_gather: k indices on both sides of the line, `out` beyond it
    pick = (np.arange(tc) * 7919) % tc
    assert len(set(pick.tolist())) == tc and (pick >= first).sum() == 41 and tc * hw > wi.LINE
    # dc_series_bin_time at b = 2: the bins have the recording's period, the last frame stays open
    assert tc % 2 == 1 and np.array_equal(gc.rows(2 * gc.K).reshape(gc.K, 2)[np.arange(200) % gc.K], gc.rows(400).reshape(200, 2))


def test_the_two_open_caps_are_crossed():
    H, W = wi.FRAME_HW
    tc, c = wi.CAP_TC, wi.BIN_C
    assert tc == 2 ** 18 + 41 and wi.BLOCK_CAP == 2 ** 28
    # dc_motion_bin: one item is 8 binned columns of one binned row; 64 x 64 binned pixels give 1024 items per frame
    per_frame = (H // c) * (-(-((W // c) * c) // 8))
    assert per_frame == 1024
    items = tc * per_frame
    assert gc.first_stride_trip(items, 1 << 20, 256) == 2 ** 28 == (tc - 41) * per_frame      # frame 2^18 opens the second trip
    assert tc * H * W * 2 // wi.GiB == 8 and tc * (H // c) * (W // c) * 2 // wi.GiB == 2
    first = wi.LINE // (H * W)
    assert first == 2 ** 17 < tc                                                     # its frames pass the line too: the line case
    f = np.arange(first, tc)
    alias = (f * H * W & wi.MASK) // (H * W)
    assert (alias < first).all() and (f % gc.K != alias % gc.K).all()
    assert (f[f >= 2 ** 18] % gc.K != (f[f >= 2 ** 18] - 2 ** 18) % gc.K).all()      # one stride of the grid early: another base frame
    assert tc * (H // c) * (W // c) <= I32_MAX                                       # `out`: 2 GiB, but not 2^31 values
    # dc_motion_block_refine
    By, Bx = wi.REFINE_BLOCKS
    items = tc * By * Bx
    assert (By, Bx) == (32, 32) and items > wi.BLOCK_CAP and gc.first_stride_trip(items, 1 << 20, 256) == 2 ** 28
    assert items * 8 // wi.GiB == 2 and items * 2 * 4 // wi.GiB == 2               # bscores at D = 0; block_shifts and fine
    assert 2 * items + 1 <= I32_MAX                                                  # the indices stay below the line: the trip is what is pinned
    assert 2 ** 18 % gc.K != 0


def test_the_table_holds_every_entry_point_the_census_finds():
    protos = _lib.parse_header()
    found = wi.census(protos)
    assert len(found) >= 45
    for name in sorted(found):
        assert (name in wi.TABLE) != (name in wi.EXEMPT), '%s: in the table or exempt, one of the two' % name
    for name, reason in wi.EXEMPT.items():
        assert name in found and name.endswith('_host') and 'stream' not in protos[name][2] and reason, name
    source = open(os.path.join(HERE, 'test_wide_index_gpu.py')).read()
    for name, (route, case, nbytes, tests) in wi.TABLE.items():
        assert name in protos and 'stream' in protos[name][2] and not name.endswith('_host'), name
        assert route and case and 0 < nbytes <= wi.BUDGET, (name, nbytes)
        for test in tests.split(', '):
            assert re.search(r'^def %s\(' % test, source, flags=re.M), (name, test)
    assert wi.BUDGET == 17 * 2 ** 30
    # what the table holds beyond the census: the cap that takes no frames, and nothing else
    assert set(wi.TABLE) - found == {'dc_motion_block_refine'}
    # every `long ld` of the census is a matrix of rows, every (frames, tc) a recording: the route says which
    for name in found & set(wi.TABLE):
        argnames = protos[name][2]
        if 'frames' in argnames:
            assert 'frame' in wi.TABLE[name][0], name
        if any(n in argnames for n in ('ld', 'ldG', 'ldH')):
            assert 'row' in wi.TABLE[name][0], name


def test_every_entry_point_that_takes_tc_answers_for_the_limit():
    protos = _lib.parse_header()
    takes_tc = {n for n, (_, argtypes, argnames) in protos.items()
                if 'tc' in argnames and 'stream' in argnames and argtypes[argnames.index('tc')] is ctypes.c_int}
    listed = [n for names in wi.TC_FAMILIES.values() for n in names]
    assert len(listed) == len(set(listed)) and set(listed) == takes_tc and len(listed) == 25
    assert {'dc_motion_block_pick', 'dc_motion_block_refine', 'dc_frame_quality'} <= takes_tc
    header = open(_lib.HEADER).read()
    assert re.search(r'^#define DC_FRAMES_PER_CALL_MAX 1073741824L$', header, flags=re.M) and wi.FRAMES_MAX == 1073741824 == 2 ** 30
    for name in listed:                                                             # the limit stands beside each prototype
        assert re.search(r'^int %s\([^;]*;\s*/\* tc <= DC_FRAMES_PER_CALL_MAX \*/' % name, header, flags=re.M), name
        module = [m for m, names in wi.TC_FAMILIES.items() if name in names][0]
        assert "check_frame_limit(dclib, '%s')" % module in open(os.path.join(HERE, module + '.py')).read(), module
    # below the limit the kernels' int arithmetic holds: the table index 2 f + 1 and the frame loop's f + gridDim.y
    f = wi.FRAMES_MAX - 1
    assert 2 * f + 1 <= I32_MAX and f + gc.FRAME_CAP <= I32_MAX and 2 * (f + 1) + 1 > I32_MAX
