"""Pure-Python mirror of the launch plans that decide how many pixel tiles (or items) ONE workgroup of the persistent
kernels walks -- no HIP, plain integer arithmetic, so the shapes of tests/test_multitile_gpu.py can be proven to enter
the multi-tile loops on a machine without a GPU (tests/test_tileplan.py) and cross-checked against the library on one.

  wgrad_plan       csrc/wgrad_f16x3.hip  CONV_H_DISPATCH / CONVT_H_DISPATCH + WgradHCfg + wgrad_h_plan
  persistent_plan  csrc/igemm_pp.hip igemm_pp_kernel, csrc/bwd_joint.hip both kernels: the per-XCD item distribution
  pp_items         csrc/igemm_pp.hip pp_launch: (pixel tile, column block) items of the role-split kernel
  joint_items      csrc/bwd_joint.hip joint_grid: pixel tiles of the joint backward kernels
  c1_plan          csrc/conv_c1.hip c1_blocks + the grid-stride loop of the first-layer weight gradient
"""

DC_WGRAD_CTAS = 256         # wgrad_f16x3.hip: one workgroup per CU, one round (a build constant, not the device's CU count)
DC_WG_RW = 4                # pixel rows per 16-wide tile of the Cin, Cout > 32 instantiation


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
