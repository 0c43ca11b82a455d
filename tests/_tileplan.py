"""Pure-Python mirror of the launch plans that decide how many pixel tiles (or items) ONE workgroup of the persistent
kernels walks -- no HIP, plain integer arithmetic, so the shapes of tests/test_multitile_gpu.py can be proven to enter
the multi-tile loops on a machine without a GPU (tests/test_tileplan.py) and cross-checked against the library on one.

  wgrad_plan       csrc/wgrad_f16x3.hip  CONV_H_DISPATCH / CONVT_H_DISPATCH + WgradHCfg + wgrad_h_plan
  persistent_plan  csrc/igemm_pp.hip igemm_pp_kernel, csrc/bwd_joint.hip both kernels: the per-XCD item distribution
  pp_items         csrc/igemm_pp.hip pp_launch: (pixel tile, column block) items of the role-split kernel
  joint_items      csrc/bwd_joint.hip joint_grid: pixel tiles of the joint backward kernels
  c1_plan          csrc/conv_c1.hip c1_blocks + the grid-stride loop of the first-layer weight gradient
  wgrad1d_plan     csrc/wgrad.hip  CONV1D_WGRAD_DISPATCH + WgradCfg + wgrad_plan (UNet1D; tests/test_spikes_multitile_gpu.py)
  conv1d_fwd_grid  csrc/spikes.hip dc_conv1d_k5_fwd: one workgroup per (trace, time tile, column block)
  quad_plan        csrc/spikes_common.h quad_blocks + the grid-stride loops of dc_conv1d_stats / dc_conv1d_k5_c1_wgrad
"""

DC_WGRAD_CTAS = 256         # wgrad_f16x3.hip: one workgroup per CU, one round (a build constant, not the device's CU count)
DC_WG_RW = 4                # pixel rows per 16-wide tile of the Cin, Cout > 32 instantiation
DC_WGRAD1D_CTAS = 512       # wgrad.hip wgrad_plan: two workgroups per CU, one resident round (a build constant too)


def cdiv(a, b):
    return (a + b - 1) // b


def wgrad_config(kind, W, Cin, Cout):
    """(TW, RW, WM, WNW, NBW) of the instantiation the dispatch macro picks (Cin / Cout: the LAYER's channel counts)."""
    if kind == 'conv':
        if W <= 8:
            return (8, 8, 2, 2, 1)
        if W <= 16:
            return (16, 4, 2, 2, 1)
        if Cin > 32 and Cout > 32:
            return (16, DC_WG_RW, 2, 2, 1)
        if Cin > 32:
            return (32, 2, 2, 1, 1)
        if Cout > 32:
            return (32, 2, 1, 2, 1)
        return (32, 2, 1, 1, 1)
    if kind == 'convT':
        if W <= 8:
            return (8, 4, 1, 2, 1)
        if Cin >= 128:
            return (16, 2, 1, 2, 2)
        return (16, 2, 1, 2, 1)
    raise ValueError(kind)


def wgrad_plan(kind, N, H, W, Cin, Cout):
    """-> (TW, TH, CM, CN, tiles_total, tiles_per_split, splits, last_split_tiles).

    The contraction runs over the pixels of the B operand (H x W for both kinds: dz for conv3x3, x for convT2x2); the
    (m, n) block is (Cin, Cout) for conv3x3 and (Cout, Cin) for convT2x2.  Workgroup `split` walks the tiles
    [split * tiles_per_split, min(.., tiles_total)): every split holds tiles_per_split tiles except the last."""
    TW, RW, WM, WNW, NBW = wgrad_config(kind, W, Cin, Cout)
    WK = 4 // (WM * WNW)
    TH = WK * RW
    CM, CN = 32 * WM, 32 * WNW * NBW
    Cm, Cn = (Cin, Cout) if kind == 'conv' else (Cout, Cin)
    tiles_total = N * cdiv(W, TW) * cdiv(H, TH)
    blocks_mn = cdiv(Cm, CM) * cdiv(Cn, CN)
    want = max(1, min(cdiv(DC_WGRAD_CTAS, blocks_mn), tiles_total))
    tiles_per_split = cdiv(tiles_total, want)
    splits = cdiv(tiles_total, tiles_per_split)
    last = tiles_total - (splits - 1) * tiles_per_split
    return TW, TH, CM, CN, tiles_total, tiles_per_split, splits, last


def wgrad_instantiation(kind, W, Cin, Cout):
    """The name the case tables use for an instantiation."""
    TW, RW, WM, WNW, NBW = wgrad_config(kind, W, Cin, Cout)
    if kind == 'conv':
        if TW == 8:
            return 'W<=8'
        if W <= 16:
            return 'W<=16'
        return '%dx%d' % (32 * WM, 32 * WNW * NBW)
    return 'W<=8' if TW == 8 else ('Cin>=128' if NBW == 2 else 'rest')


def wgrad_kernel_name(kind, W, Cin, Cout, dzin=False):
    """What dc_conv3x3_wgrad_kernel_name() spells for a conv3x3 shape with Cin > 1."""
    TW, RW, WM, WNW, NBW = wgrad_config(kind, W, Cin, Cout)
    assert kind == 'conv'
    return 'wgrad_f16x3_kernel<3,3,1,1,%d,%d,%d,%d,%d,false,%s>' % (TW, RW, WM, WNW, NBW, 'true' if dzin else 'false')


def persistent_plan(n_items, cus):
    """Items of every workgroup of a persistent launch, as a list of lists of item numbers (index: blockIdx.x).

    grid = min(n_items, cus); workgroups b and b + 8 share an XCD; XCD x owns the contiguous range of n_items // 8 items
    (one more for the first n_items % 8 XCDs) and its workgroups stride through that range."""
    G = min(n_items, cus)
    out = []
    qq, rr = n_items >> 3, n_items & 7
    for b in range(G):
        xcd, seq = b & 7, b >> 3
        nx = (G + 7 - xcd) >> 3
        xstart = xcd * (qq + 1) if xcd < rr else rr * (qq + 1) + (xcd - rr) * qq
        xcount = qq + (1 if xcd < rr else 0)
        n = (xcount - seq + nx - 1) // nx if seq < xcount else 0
        out.append([xstart + seq + j * nx for j in range(n)])
    return out


def pp_tile(Ncols):
    """(TH, TW, BN) of the role-split kernel: <4,1> for up to 32 GEMM columns, <2,2> above."""
    return (16, 32, 32) if Ncols <= 32 else (8, 32, 64)


def pp_tiles(N, H, W, Ncols):
    TH, TW, _ = pp_tile(Ncols)
    return N * cdiv(W, TW) * cdiv(H, TH)


def pp_items(N, H, W, Ncols):
    """(pixel tile, column block) items of a role-split launch with Ncols GEMM columns (Cout forward, Cin data gradient)."""
    return pp_tiles(N, H, W, Ncols) * cdiv(Ncols, pp_tile(Ncols)[2])


def joint_items(N, H, W):
    """Pixel tiles (4 rows x 32 columns) of the joint backward kernels."""
    return N * cdiv(W, 32) * cdiv(H, 4)


def c1_plan(N, H, W, Cout):
    """First-layer (Cin == 1) weight gradient -> (blocks, trips): the grid and how often its longest workgroup runs the
    grid-stride loop.  A block takes PPB = 256 / (Cout / 4) pixels a trip (the W % 4 == 0 kernel: PPB groups of 4)."""
    PPB = 256 // (Cout // 4)
    pixels = N * H * W
    blocks = min(2048, cdiv(pixels, PPB))
    units = pixels // 4 if W % 4 == 0 else pixels
    return blocks, cdiv(units, blocks * PPB)


def wgrad1d_plan(N, T, Cin, Cout):
    """UNet1D weight gradient (dc_conv1d_k5_wgrad) -> (inst, TW, CM, CN, tiles_per_trace, tiles_total, tiles_per_split, splits,
    last_split_tiles).

    A trace is an image of one row: a tile is TW samples of ONE trace (the last tile of a trace ragged when T % TW != 0), the
    (m, n) block is (Cin, Cout) in blocks of CM x CN.  Workgroup `split` walks the tiles [split * tiles_per_split,
    min(.., tiles_total)); tile t lies in trace t // tiles_per_trace and starts at sample (t % tiles_per_trace) * TW."""
    if Cin > 32 and Cout > 32:
        inst, TW, CM, CN = '64x64', 64, 64, 64
    elif Cin > 32:
        inst, TW, CM, CN = '64x32', 64, 64, 32
    elif Cout > 32:
        inst, TW, CM, CN = '32x64', 64, 32, 64
    else:
        inst, TW, CM, CN = '32x32', 128, 32, 32
    per_trace = cdiv(T, TW)
    tiles_total = N * per_trace
    blocks_mn = cdiv(Cin, CM) * cdiv(Cout, CN)
    want = max(1, min(cdiv(DC_WGRAD1D_CTAS, blocks_mn), tiles_total))
    tiles_per_split = cdiv(tiles_total, want)
    splits = cdiv(tiles_total, tiles_per_split)
    last = tiles_total - (splits - 1) * tiles_per_split
    return inst, TW, CM, CN, per_trace, tiles_total, tiles_per_split, splits, last


def conv1d_fwd_grid(N, T, Cout):
    """Workgroups of dc_conv1d_k5_fwd: one per (trace, 128-sample time tile, 64-column block).  Up to 8 the kernel's
    XCD-first map of blockIdx.x is the identity; a grid that is no multiple of 8 takes its remainder branch."""
    return N * cdiv(T, 128) * cdiv(Cout, 64)


def quad_plan(samples, C, per_lane, cap):
    """The two 1-D vector reductions (dc_conv1d_stats: per_lane 16, cap 1024; dc_conv1d_k5_c1_wgrad: 32, 512) -> (blocks,
    trips): a block holds PPB = 256 / (C / 4) sample lanes, a lane strides by blocks * PPB; past the cap trips > per_lane."""
    PPB = 256 // (C // 4)
    blocks = max(1, min(cap, cdiv(samples, PPB * per_lane)))
    return blocks, cdiv(samples, blocks * PPB)


# ---------------------------------------------------------------------------------------------------------------------
# Case tables of tests/test_multitile_gpu.py.  Weight gradients: DC_WGRAD_CTAS is a build constant, so these are the same
# on every device.  (kind, instantiation, N, H, W, Cin, Cout, tiles_per_split, last_split_tiles)
WGRAD_CASES = [
    # conv W <= 8: a tile is an image column of 8 x 8 pixels, (m, n) block 64 x 64
    ('conv', 'W<=8', 17, 3, 5, 256, 256, 2, 1),
    ('conv', 'W<=8', 65, 3, 5, 200, 96, 3, 2),
    ('conv', 'W<=8', 49, 3, 5, 256, 256, 4, 1),
    ('conv', 'W<=8', 65, 9, 5, 200, 96, 5, 5),
    # conv W <= 16: 16 x 4 pixels, 64 x 64
    ('conv', 'W<=16', 7, 12, 12, 256, 256, 2, 1),
    ('conv', 'W<=16', 33, 5, 9, 200, 96, 3, 3),
    ('conv', 'W<=16', 25, 5, 9, 256, 256, 4, 2),
    ('conv', 'W<=16', 33, 13, 9, 200, 96, 5, 2),
    # conv 64 x 64 (Cin, Cout > 32, W > 16): 16 x 4 pixels
    ('conv', '64x64', 3, 9, 33, 256, 256, 2, 1),
    ('conv', '64x64', 7, 17, 17, 200, 96, 3, 1),
    ('conv', '64x64', 5, 17, 17, 256, 256, 4, 2),
    ('conv', '64x64', 5, 33, 33, 200, 96, 5, 5),
    # conv 64 x 32 (Cin > 32 >= Cout): 32 x 4 pixels; ONE (da, z) register set when dz is formed on load
    ('conv', '64x32', 5, 17, 65, 256, 32, 2, 1),
    ('conv', '64x32', 5, 49, 33, 200, 24, 3, 1),
    ('conv', '64x32', 7, 25, 33, 512, 32, 4, 2),
    ('conv', '64x32', 5, 49, 33, 512, 24, 5, 5),
    # conv 32 x 64 (Cin <= 32 < Cout): 32 x 4 pixels; ONE (da, z) register set when dz is formed on load
    ('conv', '32x64', 5, 17, 65, 32, 256, 2, 1),
    ('conv', '32x64', 5, 49, 33, 24, 200, 3, 1),
    ('conv', '32x64', 7, 25, 33, 32, 512, 4, 2),
    ('conv', '32x64', 5, 49, 33, 24, 512, 5, 5),
    # conv 32 x 32: 32 x 8 pixels, ONE (m, n) block -> 256 splits; ONE (da, z) register set when dz is formed on load
    ('conv', '32x32', 3, 229, 66, 32, 32, 2, 1),
    ('conv', '32x32', 7, 289, 33, 24, 24, 3, 2),
    ('conv', '32x32', 7, 289, 66, 32, 32, 4, 1),
    ('conv', '32x32', 7, 289, 99, 24, 24, 5, 1),
]
CONVT_WGRAD_CASES = [
    # convT W <= 8: 8 x 8 pixels; (m, n) = (Cout, Cin), block 32 x 64
    ('convT', 'W<=8', 5, 6, 6, 512, 256, 2, 1),
    ('convT', 'W<=8', 59, 3, 5, 144, 96, 3, 2),
    ('convT', 'W<=8', 25, 3, 5, 256, 256, 4, 1),
    ('convT', 'W<=8', 59, 9, 5, 144, 96, 5, 3),
    # convT Cin >= 128: 16 x 4 pixels, block 32 x 128
    ('convT', 'Cin>=128', 9, 3, 9, 512, 256, 2, 1),
    ('convT', 'Cin>=128', 11, 13, 17, 144, 96, 3, 1),
    ('convT', 'Cin>=128', 7, 5, 9, 512, 512, 4, 2),
    ('convT', 'Cin>=128', 11, 29, 17, 144, 96, 5, 1),
    # convT rest (Cin < 128): 16 x 4 pixels, block 32 x 64
    ('convT', 'rest', 9, 9, 9, 96, 144, 2, 1),
    ('convT', 'rest', 9, 5, 17, 64, 512, 3, 3),
    ('convT', 'rest', 11, 9, 17, 96, 200, 4, 2),
    ('convT', 'rest', 9, 5, 17, 96, 512, 5, 1),
]
# first layer (Cin == 1): (N, H, W, Cout, trips of the grid-stride loop); W % 4 == 0 takes the 4-pixel kernel
C1_WGRAD_CASES = [(2, 130, 132, 256, 2), (3, 61, 63, 256, 2)]

# Case table of tests/test_spikes_multitile_gpu.py: the UNet1D weight gradient at several tiles per workgroup.
# (instantiation, N, T, Cin, Cout, tiles_per_split, last_split_tiles).  T = 5 rows: one ragged tile per trace, so every tile
# range spans several traces.  The other rows: several tiles per trace, the last ragged, their count coprime to the tiles per
# split -- ranges start and end in the middle of a trace.
WGRAD1D_CASES = [
    # 32 x 32 (Cin, Cout <= 32): 128 samples, ONE (m, n) block -> up to 512 splits, the four waves a 32-sample segment each
    ('32x32', 513, 5, 32, 32, 2, 1),
    ('32x32', 171, 330, 24, 28, 2, 1),
    ('32x32', 103, 1300, 4, 12, 3, 2),
    ('32x32', 683, 330, 4, 4, 5, 4),
    # 64 x 32 (Cin > 32 >= Cout): 64 samples, two waves per channel block, a 32-sample segment each
    ('64x32', 65, 5, 512, 32, 2, 1),
    ('64x32', 13, 270, 512, 24, 2, 1),
    ('64x32', 53, 270, 200, 24, 3, 1),
    ('64x32', 257, 5, 512, 32, 5, 2),
    # 32 x 64 (Cin <= 32 < Cout): 64 samples, as above with the roles swapped
    ('32x64', 65, 5, 32, 512, 2, 1),
    ('32x64', 13, 270, 24, 512, 2, 1),
    ('32x64', 53, 270, 24, 200, 3, 1),
    ('32x64', 257, 5, 32, 512, 5, 2),
    # 64 x 64 (Cin, Cout > 32): 64 samples, one wave per 32 x 32 block and no cross-wave sum
    ('64x64', 129, 5, 256, 256, 5, 4),
    ('64x64', 3, 700, 256, 256, 2, 1),
    ('64x64', 27, 270, 200, 96, 3, 3),
    ('64x64', 7, 450, 768, 256, 6, 2),       # the widest contraction of the real network; last tile of a trace: 2 samples
    ('64x64', 129, 270, 36, 40, 2, 1),       # ONE ragged (m, n) block: 323 splits, this instantiation's two-stage slab reduce
]
# the rows test_conv1d_k5_wgrad_multitile_probes runs: one per instantiation, several tiles per trace, a short last split, and
# enough traces for the probed ones and their neighbours to be distinct
WGRAD1D_PROBE_CASES = [WGRAD1D_CASES[i] for i in (1, 6, 10, 16)]

# the shapes of tests/test_spikes_train_gpu.py's test_conv1d_k5_wgrad (GRAD_SHAPES plus its four extra ones; the GPU module
# checks this copy against that file): ONE tile per workgroup at every one of them
WGRAD1D_DIRECT_SHAPES = [(1, 16, 4, 4), (3, 37, 12, 4), (2, 70, 32, 96), (2, 1, 4, 8), (2, 2, 8, 4),
                         (3, 5, 4, 4), (6, 200, 4, 4), (2, 70, 96, 32), (2, 70, 36, 68)]

# dc_conv1d_k5_fwd on grids past 8 workgroups: ((N, T, Cin, Cout), grid).  The (7, 5, 12, 36) launch stays below 8, where the
# XCD-first map is the identity, for contrast.
CONV1D_FWD_CASES = [((3, 260, 36, 136), 27),        # remainder 3: ragged time tile, ragged column block
                    ((5, 130, 8, 72), 20),          # remainder 4
                    ((1, 1100, 4, 200), 36),        # remainder 4: one trace, 9 time tiles
                    ((7, 5, 12, 36), 7),
                    ((2, 70, 256, 768), 24),        # remainder 0: the data gradient of the widest layer
                    ((4, 70, 256, 768), 48)]        # remainder 0, six full rounds of the 8 XCDs


def persistent_family(k, cus, H, W, Ncols=None):
    """Smallest N >= 2 for which a role-split launch (Ncols GEMM columns) or -- Ncols None -- a joint backward launch over
    N images of H x W has an item count strictly between k * cus and (k + 1) * cus that is no multiple of 8.
    -> (N, items) or None when no N fits (the per-image item count is too coarse for this device)."""
    per_img = pp_items(1, H, W, Ncols) if Ncols is not None else joint_items(1, H, W)
    for N in range(2, 4096):
        items = N * per_img
        if items >= (k + 1) * cus:
            return None
        if items > k * cus and items % 8 != 0:
            return N, items
    return None
