"""Shared by tests/test_wide_index_gpu.py (the launches), tests/test_wide_index.py (the bookkeeping, on the CPU) and the *_api.py
modules (the limit): the smallest shapes at which an element offset of a recording or trace kernel passes 2^31, the table of the
entry points that run them, and DC_FRAMES_PER_CALL_MAX, the limit behind which no test can go.  numpy only; the periodic
recordings are those of tests/_gridcaps.py (period K = 37)."""
import re

import _gridcaps as gc

K = gc.K
LINE = 1 << 31                        # the first element offset an int32 cannot hold
MASK = LINE - 1                       # what a truncating kernel keeps of a non-negative offset
GiB = 1 << 30
BUDGET = 17 * GiB                     # device bytes of one test: inputs, outputs and the expanded expectation

# ---- the row route: r * ld past the line -----------------------------------------------------------------------------------------
# (R, ld, T).  Case A: ld itself is beyond int32.  Case B: each factor fits, the product does not; row 2 starts at 2^31 + 10.
# T = 300 is a full tile of 256 frames (csrc/dff.hip, csrc/trace_dyn.hip) and a ragged one; T = 65 is one frame past the 64-frame tile
# of the deconvolution's forward walk.
ROW_A = (2, LINE + 8, 300)
ROW_B = (3, (1 << 30) + 5, 300)
ROW_B65 = (3, (1 << 30) + 5, 65)
ROW_CASES = {'A': ROW_A, 'B': ROW_B, 'B65': ROW_B65}


def row_elements(case):
    """Elements the buffer of a row-route case needs: the last row holds only its T values."""
    R, ld, T = case
    return (R - 1) * ld + T


def last_row_offset(case):
    R, ld, _ = case
    return (R - 1) * ld


def decoy_offset(case):
    """Where a kernel that keeps 31 bits of the last row's offset reads or writes: inside row 0's padding (checked on the CPU)."""
    return last_row_offset(case) & MASK


# ---- the frame route: f * H * W past the line --------------------------------------------------------------------------------------
FRAME_HW = (128, 128)
FRAME_TC = 131072 + 41                # frame 131072 is the first whose offset reaches 2^31; two grid caps of 65535 lie before it
BIN_C = 2
CAP_TC = (1 << 18) + 41               # dc_motion_bin at c = 2 and dc_motion_block_refine at 32 x 32 blocks: 1024 items per frame
REFINE_BLOCKS = (32, 32)
BLOCK_CAP = (1 << 20) * 256           # items the two kernels reach on their first trip: 2^20 workgroups of 256 threads


def frame_offset(f, HW=FRAME_HW[0] * FRAME_HW[1]):
    return f * HW


def aliased_frame(f, HW=FRAME_HW[0] * FRAME_HW[1]):
    """The frame a kernel reads that keeps 31 bits of frame f's element offset (HW divides 2^31 for the shapes here)."""
    assert LINE % HW == 0
    return (frame_offset(f, HW) & MASK) // HW


# ---- the table: entry point -> (route, case, device bytes, test of tests/test_wide_index_gpu.py) -----------------------------------
def _row_bytes(case, item, extra=0):
    return row_elements(case) * item + extra


_F = FRAME_TC * FRAME_HW[0] * FRAME_HW[1] * 2            # the frame route's recording, bytes
_SMALL = 128 << 20                                       # tables, scores and other per-frame outputs with their expectations: below 128 MiB
_C = CAP_TC * FRAME_HW[0] * FRAME_HW[1] * 2              # dc_motion_bin's recording
_I = CAP_TC * 1024                                       # dc_motion_block_refine's items

TABLE = {
    # the row route: int64 sums / numerators
    'dc_trace_combine': ('row', 'A, B', _row_bytes(ROW_A, 8, _SMALL), 'test_combine_of_rows_beyond_the_line'),
    'dc_trace_scale': ('row', 'A, B', _row_bytes(ROW_A, 8, _SMALL), 'test_scale_of_rows_beyond_the_line'),
    'dc_trace_baseline': ('row', 'A, B', _row_bytes(ROW_A, 8, _SMALL), 'test_baseline_of_rows_beyond_the_line'),
    'dc_roi_trace_finalize': ('row', 'A, B', _row_bytes(ROW_A, 8, _SMALL), 'test_finalize_of_rows_beyond_the_line'),
    'dc_roi_trace_moments': ('row', 'A, B', _row_bytes(ROW_A, 8, _SMALL), 'test_trace_moments_of_rows_beyond_the_line'),
    'dc_trace_pair_moments': ('row', 'A, B', _row_bytes(ROW_A, 8, _SMALL), 'test_pair_moments_of_rows_beyond_the_line'),
    # the row route: float32 / float64 traces
    'dc_trace_noise': ('row', 'A, B', _row_bytes(ROW_A, 8, _SMALL), 'test_noise_of_rows_beyond_the_line'),
    'dc_trace_ar1_estimate': ('row', 'A, B', _row_bytes(ROW_A, 8, _SMALL), 'test_ar1_estimate_of_rows_beyond_the_line'),
    'dc_trace_deconv_ar1': ('row', 'A, B, B65', _row_bytes(ROW_A, 8, _SMALL), 'test_deconv_of_rows_beyond_the_line'),
    'dc_trace_deconv_ar1_each': ('row', 'A, B, B65; ldG A', _row_bytes(ROW_A, 8, _SMALL), 'test_deconv_of_rows_beyond_the_line'),
    'dc_trace_deconv_ar1_base': ('row', 'A, B, B65; ldG A', _row_bytes(ROW_A, 8, _SMALL), 'test_deconv_of_rows_beyond_the_line'),
    'dc_trace_deconv_ar1_fit_base': ('row', 'A, B, B65; ldG A', _row_bytes(ROW_A, 8, _SMALL), 'test_deconv_of_rows_beyond_the_line'),
    'dc_trace_deconv_ar1_constrained': ('row', 'A, B, B65; ldG A', _row_bytes(ROW_A, 8, _SMALL), 'test_deconv_of_rows_beyond_the_line'),
    'dc_trace_deconv_ar1_constrained_base': ('row', 'A, B, B65; ldG A', _row_bytes(ROW_A, 8, _SMALL),
                                             'test_deconv_of_rows_beyond_the_line'),
    'dc_trace_deconv_search_step': ('row', 'A, B, B65; ldG A', _row_bytes(ROW_A, 8, _SMALL), 'test_deconv_of_rows_beyond_the_line'),
    'dc_trace_deconv_base_step': ('row', 'A, B, B65; ldG A', _row_bytes(ROW_A, 8, _SMALL), 'test_deconv_of_rows_beyond_the_line'),
    'dc_trace_deconv_ar2': ('row', 'A, B, B65; ldH B', _row_bytes(ROW_A, 8, _SMALL), 'test_deconv_of_rows_beyond_the_line'),
    'dc_trace_deconv_ar2_constrained': ('row', 'A, B, B65; ldH B', _row_bytes(ROW_A, 8, _SMALL), 'test_deconv_of_rows_beyond_the_line'),
    'dc_ar1_tables': ('row', 'ldG A', _row_bytes(ROW_A, 8, _SMALL), 'test_ar1_tables_of_rows_beyond_the_line'),
    # the frame route, and the ld of the three accumulators' output
    'dc_roi_trace_accumulate': ('frame + row', 'frames; sums A, B', _row_bytes(ROW_A, 8, _SMALL),
                                'test_roi_sums_of_frames_beyond_the_line, test_roi_sums_into_rows_beyond_the_line'),
    'dc_roi_wtrace_accumulate': ('frame + row', 'frames; sums A, B', _row_bytes(ROW_A, 8, _SMALL),
                                 'test_roi_sums_of_frames_beyond_the_line, test_roi_sums_into_rows_beyond_the_line'),
    'dc_roi_pixel_accumulate': ('frame + row', 'frames; sums A, B', _row_bytes(ROW_A, 8, _SMALL),
                                'test_pixel_moments_of_frames_beyond_the_line, test_pixel_moments_from_rows_beyond_the_line'),
    'dc_roi_pair_accumulate': ('frame', 'frames', _F + _SMALL, 'test_pair_sums_of_frames_beyond_the_line'),
    'dc_motion_ssd': ('frame', 'frames', _F + _SMALL, 'test_scores_of_frames_beyond_the_line'),
    'dc_motion_ssd_around': ('frame', 'frames', _F + _SMALL, 'test_window_scores_of_frames_beyond_the_line'),
    'dc_motion_block_ssd': ('frame', 'frames', _F + _SMALL, 'test_block_scores_of_frames_beyond_the_line'),
    'dc_motion_apply': ('frame', 'frames, out', 3 * _F + _SMALL, 'test_moved_frames_beyond_the_line'),
    'dc_motion_apply_sub': ('frame', 'frames, out', 3 * _F + _SMALL, 'test_moved_frames_beyond_the_line'),
    'dc_motion_warp': ('frame', 'frames, out', 3 * _F + _SMALL, 'test_moved_frames_beyond_the_line'),
    'dc_motion_warp_sub': ('frame', 'frames, out', 3 * _F + _SMALL, 'test_moved_frames_beyond_the_line'),
    'dc_bidi_scores': ('frame', 'frames', _F + _SMALL, 'test_bidi_scores_of_frames_beyond_the_line'),
    'dc_bidi_apply': ('frame', 'frames, out', 3 * _F + _SMALL, 'test_moved_frames_beyond_the_line'),
    'dc_series_accumulate': ('frame', 'frames', _F + _SMALL, 'test_series_sums_of_frames_beyond_the_line'),
    'dc_series_accumulate_xy': ('frame', 'frames', _F + _SMALL, 'test_series_sums_of_frames_beyond_the_line'),
    'dc_series_bin_time': ('frame', 'frames', _F + _F // 4 * 2 + _SMALL, 'test_time_bins_of_frames_beyond_the_line'),
    'dc_frame_moments': ('frame', 'frames', _F + _SMALL, 'test_frame_moments_beyond_the_line'),
    'dc_frame_gather': ('frame', 'frames, out', 3 * _F + _SMALL, 'test_gathered_frames_beyond_the_line'),
    # the two caps DESIGN.md 4f-caps left open; the first is dc_motion_bin's line case as well (frames AND out pass 2^31 values)
    'dc_motion_bin': ('frame + cap', 'frames, out; 2^20 x 256 items', _C + 2 * (_C // 4) + _SMALL,
                      'test_binned_frames_beyond_the_cap_and_the_line'),
    'dc_motion_block_refine': ('cap', '2^20 x 256 items; bscores, block_shifts, fine', _I * 8 * 4 + _SMALL,
                               'test_block_refine_of_items_beyond_the_cap'),
}

# What the census finds and the table does not hold, each with its reason.  Only host entry points may stand here.
_HOST = 'host twin: shares the (long)r * ld templates of the device entry point; a 16 GiB host buffer is not a unit test'
EXEMPT = {name: _HOST for name in (
    'dc_trace_deconv_ar1_host', 'dc_trace_deconv_ar1_constrained_host', 'dc_trace_deconv_ar1_fit_base_host',
    'dc_trace_deconv_ar1_constrained_base_host', 'dc_trace_deconv_ar2_host', 'dc_trace_deconv_ar2_constrained_host',
    'dc_trace_ar1_estimate_host')}


def census(protos):
    """The entry points of the header (deep_calcium_amd._lib.parse_header()) whose addresses can pass the line in one call: those
    that take (frames, tc) and those that take a `long ld`, `ldG` or `ldH`."""
    import ctypes
    found = set()
    for name, (_, argtypes, argnames) in protos.items():
        if 'frames' in argnames and 'tc' in argnames:
            found.add(name)
        for t, n in zip(argtypes, argnames):
            if n in ('ld', 'ldG', 'ldH') and t is ctypes.c_long:
                found.add(name)
    return found


# ---- the limit no test can reach: DC_FRAMES_PER_CALL_MAX -------------------------------------------------------------------------
FRAMES_MAX = 1 << 30
# every device entry point that takes `int tc`, by the *_api.py module that checks its refusal
TC_FAMILIES = {
    'test_motion_api': ('dc_motion_ssd', 'dc_motion_pick', 'dc_motion_apply'),
    'test_motion_block_api': ('dc_motion_block_ssd', 'dc_motion_block_pick', 'dc_motion_warp'),
    'test_motion_sub_api': ('dc_motion_refine', 'dc_motion_block_refine', 'dc_motion_apply_sub', 'dc_motion_warp_sub'),
    'test_motion_wide_api': ('dc_motion_bin', 'dc_motion_ssd_around', 'dc_motion_pick_around'),
    'test_bidi_api': ('dc_bidi_scores', 'dc_bidi_apply'),
    'test_series_api': ('dc_series_accumulate', 'dc_series_accumulate_xy'),
    'test_tbin_api': ('dc_series_bin_time',),
    'test_traces_api': ('dc_roi_trace_accumulate',),
    'test_weighted_api': ('dc_roi_wtrace_accumulate',),
    'test_footprints_api': ('dc_roi_pixel_accumulate',),
    'test_roi_pairs_api': ('dc_roi_pair_accumulate',),
    'test_frames_api': ('dc_frame_moments', 'dc_frame_quality', 'dc_frame_gather'),
}
_P = 1 << 44                          # an aligned non-null value; the buffers lie 2^44 bytes apart, so none overlaps another
_INTS = dict(is_unsigned=0, H=40, W=50, S=2, D=1, By=1, Bx=1, fill=0, mult=1, c=2, P=1, p=0, b=2, phase=0, k=1, y0=0, y1=40, x0=0, x1=50,
             n=2000, ta=0, tb=1, t0=0, n_total=1 << 31, R=1, N=1, ntiles=1, G=1, ld=1 << 31)


def _limit_args(protos, name, tc, odd):
    """Valid arguments for `name` with this tc; odd: the first pointer is off by one byte, which every entry point refuses with
    DC_EINVAL AFTER it has looked at tc and before it launches."""
    import ctypes
    _, argtypes, argnames = protos[name]
    args, pointers = [], 0
    for t, n in zip(argtypes, argnames):
        if n == 'stream':
            args.append(None)
        elif n == 'tc':
            args.append(tc)
        elif t is ctypes.c_void_p:
            pointers += 1
            args.append(_P * pointers + (1 if odd and pointers == 1 else 0))
        else:
            args.append(1 if n == 'S' and 'row_off' in argnames else _INTS[n])        # S: CSR rows there, a search radius elsewhere
    return args


def check_frame_limit(dclib, module):
    """tc = 2^30 + 1 is refused with DC_EUNSUP (-3) and the limit's message; tc = 2^30 passes that check (the call is then refused for its
    misaligned first pointer: nothing may be launched here).  For the entry points the module `module` answers for."""
    import pytest
    from deep_calcium_amd._lib import DcunetError
    protos = dclib.protos
    for name in TC_FAMILIES[module]:
        with pytest.raises(DcunetError, match=r'\(-3\).*%s: tc = 1073741825: the frames of one call are limited to 2\^30 = 1073741824' % name):
            getattr(dclib, name)(*_limit_args(protos, name, FRAMES_MAX + 1, False))
        with pytest.raises(DcunetError, match=r'\(-1\)') as e:
            getattr(dclib, name)(*_limit_args(protos, name, FRAMES_MAX, True))
        assert 'frames of one call' not in str(e.value) and re.search('misaligned|aligned', str(e.value)), (name, str(e.value))
