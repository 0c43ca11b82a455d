"""Shared by tests/test_grid_caps_gpu.py (the launches) and tests/test_grid_caps.py (the bookkeeping, on the CPU): the caps of the
recording kernels' grids, the shapes that cross them, periodic recordings whose oracle costs K frames, and two vectorised
oracles (the rolling percentile at half-width 1, the ROI sums).  numpy only."""
import numpy as np

# ---- the caps (csrc/motion.hip, csrc/traces.hip, csrc/dff.hip) -----------------------------------------------------------------
FRAME_CAP = 65535                     # frame_dim(tc), kMaxY, the tile dimension of dc_roi_trace_accumulate
ITEM_CAP = 1 << 20                    # workgroups of dc_motion_block_pick
APPLY_X_CAP = 4096                    # workgroups along x of dc_motion_apply(_sub): 256 threads x 8 values each
ZERO_CAP = 1024 * 256                 # values the zero kernels clear in one trip (kZeroBlocks x 256 threads)
TRACE_TILE = 32                       # frames per workgroup of dc_roi_trace_accumulate
DFF_TILE = 256                        # frames per workgroup of dc_trace_combine / dc_trace_scale / dc_trace_baseline

# ---- the shapes that cross them ------------------------------------------------------------------------------------------------
TWO_TRIPS = FRAME_CAP + 41            # frames: the last 41 are a second trip
THREE_TRIPS = 2 * FRAME_CAP + 3       # frames: the last 3 are a third trip
TRACE_FRAMES = FRAME_CAP * TRACE_TILE + 70        # 65535 tiles of 32 frames and three more
DFF_FRAMES = FRAME_CAP * DFF_TILE + 300           # 65535 tiles of 256 frames and two more
BIG_H, BIG_W = 2051, 4099             # one frame of more than 8 * 4096 * 256 values: dc_motion_apply's x grid strides
BIG_BAND = 8                          # output rows [BIG_H - 8, BIG_H) hold every second-trip group (test_grid_caps.py)

K = 37                                # period of the recordings: divides neither 65535 = 3 * 5 * 17 * 257 nor a power of two


def rows(n):
    """The base item behind each of n items: f % K."""
    return np.arange(n, dtype=np.int64) % K


def expand(base, n):
    """n items, item f = base[f % K]."""
    base = np.asarray(base)
    assert base.shape[0] == K
    return base[rows(n)]


def base_frames(rs, shape, dtype):
    """K distinct random frames over the whole range of dtype; both extremes are planted in the first and the last frame."""
    info = np.iinfo(dtype)
    f = rs.randint(info.min, info.max + 1, size=(K,) + tuple(shape)).astype(dtype)
    f[0].flat[0], f[0].flat[-1] = info.min, info.max
    f[-1].flat[0], f[-1].flat[-1] = info.max, info.min
    assert len({a.tobytes() for a in f}) == K
    return f


def first_stride_trip(n, cap, per=1):
    """The first of n items that a grid of `cap` workgroups, `per` items each, reaches on a second trip; None: one trip."""
    return cap * per if n > cap * per else None


# ---- vectorised oracles ----------------------------------------------------------------------------------------------------------
def baseline_half1(num, q):
    """The rolling percentile of include/dcunet.h at half-width 1, (R, T) int64 -> (R, T) int64: the three shifted copies of the
    trace sorted per frame, a sentinel above every value where the window is clipped, rank (q (n - 1)) // 100 with n the
    window's length (2 at the two ends, 1 for a single frame)."""
    num = np.asarray(num, np.int64)
    R, T = num.shape
    sentinel = np.iinfo(np.int64).max
    assert num.max() < sentinel
    w = np.full((3, R, T), sentinel, np.int64)
    w[1] = num
    w[0, :, 1:] = num[:, :-1]
    w[2, :, :-1] = num[:, 1:]
    w.sort(axis=0)
    n = np.full(T, 3, np.int64)
    n[0] -= 1
    n[-1] -= 1
    k = (q * (n - 1)) // 100
    return np.take_along_axis(w, np.broadcast_to(k[None, None, :], (1, R, T)), axis=0)[0]


def roi_sums(frames, pixels):
    """(len(pixels), t) int64: the sum of the flat pixel indices of every list, per frame."""
    flat = np.asarray(frames).reshape(len(frames), -1).astype(np.int64)
    return np.stack([flat[:, np.asarray(p, np.int64)].sum(axis=1) for p in pixels])


def apply_second_trip_rows(H, W, tc):
    """The output rows of dc_motion_apply(_sub) that hold a value of a second-trip group, over the tc frames of a launch: group g
    of frame t covers the values [8 g - off, 8 g - off + 8) of the frame, off = (t H W) & 7, and the groups from
    APPLY_X_CAP * 256 on are second-trip.  -> (first row, last row) or None."""
    first = None
    for t in range(tc):
        off = (t * H * W) & 7
        groups = (H * W + off + 7) // 8
        if groups > APPLY_X_CAP * 256:
            e = max(0, APPLY_X_CAP * 256 * 8 - off)
            first = e // W if first is None else min(first, e // W)
    return None if first is None else (first, H - 1)
