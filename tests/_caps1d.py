"""Shared by tests/test_caps1d_gpu.py (the launches) and tests/test_caps1d.py (the bookkeeping, on the CPU): the grid cap of the six
grid-stride launches of the UNet1D kernels (spikes_blocks() of csrc/spikes_common.h), the number of float4 items each entry point
hands its kernel, the (trace, sample, channel quad) a flat item stands for under each kernel's decomposition, and the shapes of the
GPU module with the regime each one claims.  numpy only."""
import numpy as np

# ---- the cap (csrc/spikes_common.h: spikes_blocks(total, cap = 8192), every launch 256 threads) ---------------------------------------
CAP_BLOCKS = 8192
THREADS = 256
CAP_ITEMS = CAP_BLOCKS * THREADS      # 2 097 152 float4 items per trip of a capped launch

# entry point -> (kernel, source file): the ONLY users of spikes_blocks()
LAUNCHES = {
    'dc_conv1d_k5_c1_fwd': ('conv1d_k5_c1_kernel', 'spikes.hip'),
    'dc_maxpool1d_2_fwd': ('maxpool1d_2_kernel', 'spikes.hip'),
    'dc_upsample1d_2x_fwd': ('upsample1d_2x_drop_fwd_kernel', 'spikes.hip'),
    'dc_upsample1d_2x_drop_fwd': ('upsample1d_2x_drop_fwd_kernel', 'spikes.hip'),
    'dc_upsample1d_2x_drop_bwd': ('upsample1d_2x_drop_bwd_kernel', 'spikes.hip'),
    'dc_maxpool1d_2_bwd': ('maxpool1d_2_bwd_kernel', 'spikes_train.hip'),
}
UP = ('dc_upsample1d_2x_fwd', 'dc_upsample1d_2x_drop_fwd', 'dc_upsample1d_2x_drop_bwd')


def rows(entry, T):
    """Samples (or sample pairs) per trace the kernel of `entry` walks: T for the first layer and for the up-sampling (T is the
    length BEFORE up-sampling), floor(T / 2) output samples for the pooling, ceil(T / 2) input pairs for its backward (the last
    one of an odd T is a single sample)."""
    if entry == 'dc_maxpool1d_2_fwd':
        return T // 2
    if entry == 'dc_maxpool1d_2_bwd':
        return (T + 1) // 2
    assert entry == 'dc_conv1d_k5_c1_fwd' or entry in UP, entry
    return T


def total(entry, N, T, C):
    """`total` of the launch: float4 items, one per thread and trip."""
    assert C % 4 == 0
    return N * rows(entry, T) * (C // 4)


def blocks(items):
    """spikes_blocks()."""
    return max(1, min(CAP_BLOCKS, -(-items // THREADS)))


def trips(items):
    """(trips of the first thread, trips of the last thread of the last workgroup) of `for (i = tid; i < items; i += lanes)`."""
    lanes = blocks(items) * THREADS
    return -(-items // lanes), max(0, -(-(items - (lanes - 1)) // lanes))


def trip_of(i, items):
    """The trip (0 = first) on which flat item i of a launch of `items` is done."""
    return i // (blocks(items) * THREADS)


def decompose(entry, i, N, T, C):
    """(n, t, cg) of flat item i as the kernel forms them: cg = i % C4, s = i / C4, n = s / rows, t = s % rows.  t counts what
    rows() counts: the sample of the first layer, the INPUT sample of the up-sampling (outputs 2t and 2t + 1), the OUTPUT sample
    of the pooling (inputs 2t and 2t + 1), the input pair of the pooling's backward (samples 2t and, if 2t + 1 < T, 2t + 1)."""
    C4, R = C // 4, rows(entry, T)
    assert 0 <= i < N * R * C4
    s = i // C4
    return s // R, s % R, i % C4


def item_of(entry, n, t, c, N, T, C):
    """The flat item that owns channel c of row t (in the units of rows()) of trace n: the inverse of decompose()."""
    return (n * rows(entry, T) + t) * (C // 4) + c // 4


def first_mismatch(entry, bad, N, T, C):
    """bad: boolean (N, samples, C) over an OUTPUT of `entry`, True where the device is wrong.  -> None, or a sentence naming the
    first wrong flat item (in item order), its (n, t, cg), its trip and how many elements are wrong.  `samples` per row of
    rows(): 2 for the up-sampling forward and the pooling backward (whose last pair may be single), 1 otherwise."""
    bad = np.asarray(bad)
    if not bad.any():
        return None
    R, C4 = rows(entry, T), C // 4
    per = 2 if entry in ('dc_upsample1d_2x_fwd', 'dc_upsample1d_2x_drop_fwd', 'dc_maxpool1d_2_bwd') else 1
    n, u = [int(v) for v in np.argwhere(bad.any(axis=2))[0]]            # C order: the first (n, sample), hence the first (n, t)
    t = u // per
    quads = bad[n, t * per:t * per + per].reshape(-1, C4, 4).any(axis=(0, 2))
    i = item_of(entry, n, t, 4 * int(np.flatnonzero(quads)[0]), N, T, C)
    items = N * R * C4
    return ('%s N=%d T=%d C=%d: %d wrong elements, the first in flat item %d = (n %d, t %d, quad %d) of %d, trip %d of %d'
            % (entry, N, T, C, int(bad.sum()), i, n, t, i % C4, items, trip_of(i, items) + 1, trips(items)[0]))


# ---- the cases: (regime, N, T, C) ---------------------------------------------------------------------------------------------------
# 'cap+1'  total == CAP_ITEMS + 1: the one second-trip item is quad 2 of the last row of the last trace; C = 12, so C4 = 3 does not
#          divide the stride and a thread would change its quad on every trip
# 'third'  2 CAP_ITEMS < total < 2.01 CAP_ITEMS: a short ragged third trip; C4 divides the stride (C = 32) or not (C = 24)
# 'short'  traces of 3 samples, shorter than the 5-tap kernel: every tap of every sample looks at a halo, most of them on the second trip
CASES = {
    'dc_conv1d_k5_c1_fwd': [('cap+1', 3, 233017, 12), ('third', 2, 350003, 24), ('short', 200003, 3, 16)],
    'dc_maxpool1d_2_fwd': [('cap+1', 3, 466035, 12), ('third', 5, 209801, 32)],
    'dc_maxpool1d_2_bwd': [('cap+1', 3, 466033, 12), ('third', 5, 209800, 32)],
    'dc_upsample1d_2x_fwd': [('cap+1', 3, 233017, 12), ('third', 5, 104900, 32)],
}
CASES['dc_upsample1d_2x_drop_fwd'] = CASES['dc_upsample1d_2x_drop_bwd'] = CASES['dc_upsample1d_2x_fwd']
PAD = 4                               # every sample stride a case passes is C + PAD, the slice at channel offset PAD
RNG_SMALL = (2, 5, 8)                 # (N, T, C) of the small-shape pin of the counter RNG: one workgroup, no cap in sight
MAX_BUFFER_BYTES = 256 * 10 ** 6


def case_ids(entry):
    return ['%s-N%d-T%d-C%d' % c for c in CASES[entry]]


def buffers(entry, N, T, C):
    """{name: bytes} of every device buffer a case of `entry` allocates (guards aside)."""
    ld = C + PAD
    if entry == 'dc_conv1d_k5_c1_fwd':
        return dict(x=4 * N * T, y=4 * N * T * ld)
    if entry == 'dc_maxpool1d_2_fwd':
        return dict(inp=4 * N * T * ld, out=4 * N * (T // 2) * C)
    if entry == 'dc_maxpool1d_2_bwd':
        return dict(dy=4 * N * (T // 2) * C, inp=4 * N * T * ld, skip=4 * N * T * ld, dx=4 * N * T * ld)
    if entry == 'dc_upsample1d_2x_drop_bwd':
        return dict(dout=4 * N * 2 * T * ld, mask=N * 2 * T * C, din=4 * N * T * C)
    return dict(inp=4 * N * T * C, out=4 * N * 2 * T * ld, mask=N * 2 * T * C)


# ---- the engine-level case ---------------------------------------------------------------------------------------------------------
ENGINE = dict(nfb=4, margin=4, T=4096, B=1101, sub=256, model_seed=15, trace_seed=11, oracle_traces=(0, 1, 1023, 1024, 1099, 1100))
CONV_TT, CONV_BN, HEAD_TT = 128, 64, 192          # csrc/spikes.hip CONV1D_CFG (4 x 1 x 32 samples, 1 x 2 x 32 columns); HEAD_TT


def engine_launches(B, T, nfb):
    """What UNet1DEngine.forward launches for B traces of T samples (deep_calcium_amd/unet1d.py, _run):
    -> (capped [(entry, N, T, C)], dc_conv1d_k5_fwd grids [workgroups], dc_spike_head_fwd workgroups)."""
    capped, grids = [], []

    def conv(ci, co, t):
        if ci == 1:
            capped.append(('dc_conv1d_k5_c1_fwd', B, t, co))
        else:
            grids.append(B * -(-t // CONV_TT) * -(-co // CONV_BN))

    cin = 1
    for lvl in range(5):
        c, t = nfb << lvl, T >> lvl
        if lvl:
            capped.append(('dc_maxpool1d_2_fwd', B, 2 * t, c >> 1))
        conv(cin, c, t)
        conv(c, c, t)
        cin = c
    for lvl in (3, 2, 1, 0):
        c, t = nfb << lvl, T >> lvl
        capped.append(('dc_upsample1d_2x_fwd', B, t >> 1, 2 * c))
        conv(3 * c, c, t)
        conv(c, c, t)
    return capped, grids, B * -(-T // HEAD_TT)
