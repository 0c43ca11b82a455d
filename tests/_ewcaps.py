"""Shared by tests/test_ew_caps_gpu.py (the launches) and tests/test_ew_caps.py (the bookkeeping, on the CPU): the grid caps of
csrc/elementwise.hip as the source states them, the trip counts a shape gives the first and the last thread of a launch, the
shapes of the GPU module with the regime each one claims, and the numpy oracle of dc_crop_augment.  numpy only."""
import numpy as np

# ---- the caps (csrc/elementwise.hip) -------------------------------------------------------------------------------------------
THREADS = 256                         # every kernel of the file runs 256 threads per workgroup, one item per thread and trip
K_MAX_BLOCKS = 1280                   # kMaxBlocks = kMaxBwdBlocks: dc_bn_relu_drop_fwd, dc_bn_relu_drop_pool_fwd, dc_bn_bwd_*
CAP_4096 = 4096                       # dc_maxpool2x2_fwd / _bwd, dc_upsample2x_drop_fwd / _bwd, dc_adam_step_flat, dc_gather_maps,
                                      # dc_tta_merge
CAP_2048 = 2048                       # dc_maxpool2x2_bwd_bnred, dc_fill, dc_scale_flat
HEAD_CAP = 1024                       # dc_head_blocks
CROP_CAP = 64                         # dc_crop_augment: workgroups per image, a thread takes 4 pixels of a row
ROUND_CAP = 256                       # dc_round_window_u8: workgroups per map
ADAM_VEC = 4                          # dc_adam_step_flat: parameters per thread and trip; n % 4 more in workgroup 0


def ppb(C):
    """Pixels per workgroup of the pixel-lane kernels: 256 threads = PPB pixel lanes x C / 4 channel quads."""
    assert C % 4 == 0 and THREADS % (C // 4) == 0
    return THREADS // (C // 4)


def bn_blocks(pixels, C, cap=K_MAX_BLOCKS):
    """ew_blocks(): the grid of the pixel-lane kernels."""
    return max(1, min(cap, -(-pixels // ppb(C))))


def bn_stride(C):
    """Pixels one trip of a capped pixel-lane launch covers: 1280 x 1024 / C, whatever C is 1 310 720 floats per tensor."""
    return K_MAX_BLOCKS * ppb(C)


def flat_blocks(items, cap):
    """The grid of the flat kernels: one item per thread."""
    return max(1, min(cap, -(-items // THREADS)))


def lane_trips(items, lanes):
    """Trips of a grid-stride loop `for (i = lane; i < items; i += lanes)`: (of lane 0, of the last lane)."""
    return -(-items // lanes), max(0, -(-(items - (lanes - 1)) // lanes))


def flat_trips(items, cap):
    """(trips of the first thread, trips of the last thread of the last workgroup) of a flat kernel."""
    return lane_trips(items, flat_blocks(items, cap) * THREADS)


def bn_trips(pixels, C):
    """The same for the pixel lanes of dc_bn_relu_drop_fwd."""
    return lane_trips(pixels, bn_blocks(pixels, C) * ppb(C))


def sweep_census(pixels, C):
    """bn_bwd_sweep: a pixel lane with n pixels runs n // 2 two-pixel bodies and n % 2 tails.  {(bodies, tails): lanes}."""
    lanes = bn_blocks(pixels, C) * ppb(C)
    q, r = divmod(pixels, lanes)
    census = {}
    for n, count in ((q + 1, r), (q, lanes - r)):
        if count:
            key = (n // 2, n % 2)
            census[key] = census.get(key, 0) + count
    return census


def sweep_trips(pixels, C):
    """((bodies, tails) of the first pixel lane, of the last one)."""
    lanes = bn_blocks(pixels, C) * ppb(C)
    first, last = lane_trips(pixels, lanes)
    return (first // 2, first % 2), (last // 2, last % 2)


# ---- the BatchNorm passes: P in units of s = bn_stride(C) ----------------------------------------------------------------------
def bn_pixels(regime, C):
    s = bn_stride(C)
    return [s + 1, 3 * s // 2 + 3, 2 * s, 2 * s + 1, 5 * s // 2 + 3, 7 * s // 2 + 3][regime]


# what sweep_trips() must give per regime, and in words
BN_REGIMES = [
    (((1, 0), (0, 1)), 'one lane with a body trip, the rest tail-only'),
    (((1, 0), (0, 1)), 'half the lanes a body trip, half a tail'),
    (((1, 0), (1, 0)), 'body trips, no tail anywhere'),
    (((1, 1), (1, 0)), 'exactly one tail'),
    (((1, 1), (1, 0)), 'one body trip then a tail'),
    (((2, 0), (1, 1)), 'two body trips beside one body trip plus a tail'),
]
# (regime, C, dropout, pixel stride of da / of the forward's output).  C = 32 takes every regime, 4 and 1024 (PPB 256 and 1) three
# each, so that every regime meets two widths; each dropout kind meets every width.
BN_CASES = [(0, 32, 'none', 40), (1, 32, 'mask', 64), (2, 32, 'rng', 40), (3, 32, 'none', 32), (4, 32, 'mask', 40), (5, 32, 'rng', 64),
            (0, 4, 'rng', 12), (2, 4, 'mask', 4), (4, 4, 'none', 8),
            (1, 1024, 'mask', 1024), (3, 1024, 'none', 1032), (5, 1024, 'rng', 2048)]
BN_EXTRA = 1003                       # pixels of the other data-parallel shard: count = pixels + BN_EXTRA in dc_bn_bwd_apply_count

# ---- the flat kernels: (N, H, W, C) and friends --------------------------------------------------------------------------------
POOL_FUSED_SHAPES = [(5, 192, 184, 32), (5, 264, 256, 32), (6, 480, 472, 4)]      # dc_bn_relu_drop_pool_fwd: 1.08, 2.06, 1.04 trips
POOL_SHAPE = (3, 954, 954, 8)                                                     # dc_maxpool2x2_fwd / _bwd: 1.30 trips, ragged
POOL_BNRED_SHAPES = [(2, 1040, 1040, 8), (1, 260, 260, 256)]                      # dc_maxpool2x2_bwd_bnred: 2.06 trips
ADAM_TRIP = CAP_4096 * THREADS * ADAM_VEC                                         # 4 194 304 parameters
ADAM_N = [2 * ADAM_TRIP + 4099 + 3, 2 * ADAM_TRIP + 4099]                         # n % 4 = 2 and 3: third trip, scalar tail
FILL_N = CAP_2048 * THREADS + 77
TTA = dict(H=1040, W=1040, hs=1031, ws=1027, K=2)
CROP_HW = [260, 512]
ROUND = dict(N=2, H=264, W=260, y0=3, y1=261, x0=2, x1=257)


def pool_items(N, H, W, C):
    return N * (H // 2) * (W // 2) * (C // 4)


def crop_threads(hw):
    """Threads' worth of work per image of dc_crop_augment: 4 pixels of a row each."""
    return hw * (hw // 4)


# ---- dc_crop_augment in numpy ---------------------------------------------------------------------------------------------------
def d4_apply(win, d4):
    """out[i][j] = win[r][c], (r, c) = (d4 & 1) ? (j, i) : (i, j); r -> n-1-r if d4 & 2; c -> n-1-c if d4 & 4 (include/dcunet.h),
    as numpy flips and a transpose."""
    if d4 & 2:
        win = win[::-1, :]
    if d4 & 4:
        win = win[:, ::-1]
    return win.T if d4 & 1 else win


def crop_ref(S, y0, x0, eh, ew, hw, d4):
    """The zero-filled (hw, hw) window of S[y0 : y0 + eh, x0 : x0 + ew], then the dihedral map."""
    win = np.zeros((hw, hw), S.dtype)
    win[:eh, :ew] = S[y0:y0 + eh, x0:x0 + ew]
    return np.ascontiguousarray(d4_apply(win, d4))


def crop_items(hw, shape, rs):
    """16 items on a source image of `shape`: every d4 on a full window, every d4 on a crop smaller than the window (one of them
    empty, one a single row, one a single column).  -> [(y0, x0, eh, ew, d4)]"""
    Hs, Ws = shape
    items = []
    for d4 in range(8):
        items.append((int(rs.randint(0, Hs - hw + 1)), int(rs.randint(0, Ws - hw + 1)), hw, hw, d4))
    short = [(hw - 1, hw), (hw, hw - 3), (hw // 2 + 1, hw // 3), (1, hw), (hw, 1), (0, 0), (7, 5), (hw - 5, hw - 2)]
    for d4, (eh, ew) in enumerate(short):
        items.append((int(rs.randint(0, Hs - hw + 1)), int(rs.randint(0, Ws - hw + 1)), eh, ew, d4))
    return items
