"""The ROI pixel-pair correlation restated for the tests (include/dcunet.h, "ROI pixel-pair correlation"): moments in Python
integers, corr by the formula with float(int) (correctly rounded, like dc_i128_to_f64) and math.sqrt, an independent 60-digit
decimal evaluation of the exact quotient, the tile list, the split rule naively in Python lists, and the scenes of the tests.
Shares no code with the product."""
import decimal
import math

import numpy as np

TILE = 64


# ---- moments and corr ------------------------------------------------------------------------------------------------------
def moments(frames, flat):
    """frames (T,H,W), flat: the ROI's flat pixel indices in order -> (a list[k], g list[k][k]) of Python ints, g full and symmetric."""
    T = frames.shape[0]
    cols = [[int(v) for v in frames.reshape(T, -1)[:, p]] for p in flat]
    a = [sum(c) for c in cols]
    k = len(cols)
    g = [[0] * k for _ in range(k)]
    for i in range(k):
        for j in range(i, k):
            g[i][j] = g[j][i] = sum(x * y for x, y in zip(cols[i], cols[j]))
    return a, g


def numerators(T, a, g, i, j):
    return T * g[i][i] - a[i] * a[i], T * g[i][j] - a[i] * a[j], T * g[j][j] - a[j] * a[j]


def corr64(T, a, g, i, j):
    """The contract's formula in doubles, before the rounding to float32."""
    cii, cij, cjj = numerators(T, a, g, i, j)
    if cii <= 0 or cjj <= 0:
        return 0.0
    return float(cij) / (math.sqrt(float(cii)) * math.sqrt(float(cjj)))


_CTX = decimal.Context(prec=60)


def corr_exact(T, a, g, i, j):
    """Cij / sqrt(Cii Cjj) in 60-digit decimal arithmetic, rounded once (decimal -> double -> float32; the double step moves the
    result by < 2^-29 float32 ulp)."""
    cii, cij, cjj = numerators(T, a, g, i, j)
    if cii <= 0 or cjj <= 0:
        return np.float32(0)
    return np.float32(float(_CTX.divide(decimal.Decimal(cij), _CTX.sqrt(decimal.Decimal(cii * cjj)))))


def matrix(T, a, g, fn=corr_exact):
    k = len(a)
    return np.array([[fn(T, a, g, i, j) for j in range(k)] for i in range(k)], np.float32 if fn is corr_exact else np.float64).reshape(k, k)


# ---- bookkeeping -----------------------------------------------------------------------------------------------------------
def layout(areas):
    """-> (roi_off, goff, tiles, G) as plain lists, by the header's words: every (r, ti, tj) with ti <= tj < ceil(k / TILE)."""
    roi_off, goff, tiles, G = [0], [], [], 0
    for r, k in enumerate(areas):
        roi_off.append(roi_off[-1] + k)
        goff.append(G)
        G += k * k
        nt = -(-k // TILE)
        for ti in range(nt):
            for tj in range(nt):
                if ti <= tj:
                    tiles.append((r, ti, tj))
    return roi_off, goff, tiles, G


# ---- the split rule, naively -------------------------------------------------------------------------------------------------
def _dist2(u, v):
    return sum((x - y) ** 2 for x, y in zip(u, v))


def _components(points, W):
    """8-connected components of a set of (y, x) by flood fill, each sorted by flat index, in the order of their smallest one."""
    left = set(points)
    comps = []
    while left:
        seed = min(left, key=lambda p: p[0] * W + p[1])
        left.remove(seed)
        comp, todo = [seed], [seed]
        while todo:
            y, x = todo.pop()
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    q = (y + dy, x + dx)
                    if q in left:
                        left.remove(q); comp.append(q); todo.append(q)
        comps.append(sorted(comp, key=lambda p: p[0] * W + p[1]))
    return comps


def split_one(c, C, W, min_gap, min_area, iterations):
    """c: list of (y, x) in flat order; C: k x k nested lists of floats.  -> (parts or None, gap or nan)."""
    k = len(c)
    rowsum = [sum(C[i]) for i in range(k)]
    i0 = max(range(k), key=lambda i: (rowsum[i], -i))
    d = [_dist2(C[j], C[i0]) for j in range(k)]
    j0 = max(range(k), key=lambda j: (d[j], -j))
    c0, c1 = list(C[i0]), list(C[j0])
    labels = None
    for _ in range(iterations):
        new = [1 if _dist2(C[i], c1) < _dist2(C[i], c0) else 0 for i in range(k)]
        if new == labels:
            break
        labels = new
        if sum(new) in (0, k):
            return None, float('nan')
        rows0, rows1 = [C[i] for i in range(k) if not new[i]], [C[i] for i in range(k) if new[i]]
        c0 = [sum(col) / len(rows0) for col in zip(*rows0)]
        c1 = [sum(col) / len(rows1) for col in zip(*rows1)]
    where = dict((p, n) for n, p in enumerate(c))
    parts = []
    for side in (0, 1):
        comps = _components([c[i] for i in range(k) if labels[i] == side], W)
        parts.append(max(comps, key=lambda g: (len(g), -(g[0][0] * W + g[0][1]))))
    if min(len(p) for p in parts) < 2:
        return None, float('nan')
    ix = [[where[p] for p in part] for part in parts]
    within = [sum(C[i][j] for i in m for j in m if i != j) / (len(m) * (len(m) - 1)) for m in ix]
    between = sum(C[i][j] for i in ix[0] for j in ix[1]) / (len(ix[0]) * len(ix[1]))
    gap = min(within) - between
    if min(len(p) for p in parts) < min_area or not gap >= min_gap:
        return None, gap
    parts.sort(key=lambda p: p[0][0] * W + p[0][1])
    return parts, gap


def split(pixels, corr, shape, min_gap=0.1, min_area=8, iterations=16):
    H, W = shape
    new, origin, gaps = [], [], []
    for r, (c, C) in enumerate(zip(pixels, corr)):
        c = [(int(y), int(x)) for y, x in c]
        parts, gap = None, float('nan')
        if C is not None and len(c) >= 2 * min_area:
            parts, gap = split_one(c, [[float(v) for v in row] for row in np.asarray(C, np.float64)], W, min_gap, min_area, iterations)
        gaps.append(gap)
        for p in ([c] if parts is None else parts):
            new.append(np.array(p, np.int64).reshape(-1, 2))
            origin.append(r)
    return new, origin, np.array(gaps, np.float64)


# ---- the scenes of the tests -------------------------------------------------------------------------------------------------
SCENES = ('two', 'same', 'gauss', 'static')
REGION = (2, 2, 6, 12)                # y0, x0, height, width of the region inside the frame


def _activity(rs, T, rate=0.03, decay=8.0):
    spikes = rs.poisson(rate, T).astype(np.float64)
    return np.convolve(spikes, np.exp(-np.arange(T) / decay))[:T], int(spikes.sum())


def scene(kind, seed, amplitude=60.0, sigma=30.0, T=256, shape=(10, 16)):
    """One 6 x 12 region in a frame of `shape`, int16, baseline 400, a shared neuropil trace at 0.3 * amplitude, Gaussian pixel
    noise: 'two' -- two 6 x 6 cells side by side with independent Poisson activity (rate 0.03, decay 8 frames); 'same' -- one
    cell, both halves the same trace; 'gauss' -- one cell whose amplitude falls off as a Gaussian from the region's centre;
    'static' -- no activity.  -> frames (T,H,W), the region's (72,2) [y,x], the left and the right half's pixels, and how many
    events the left and the right activity hold (the right one is used by 'two' only)."""
    rs = np.random.RandomState(1000 * SCENES.index(kind) + seed)
    H, W = shape
    y0, x0, h, w = REGION
    (s1, n1), (s2, n2), (npil, _) = _activity(rs, T), _activity(rs, T), _activity(rs, T)
    f = 400.0 + 0.3 * amplitude * npil[:, None, None] * np.ones((1, H, W))
    amp = np.zeros((2, H, W))
    if kind == 'two':
        amp[0, y0:y0 + h, x0:x0 + w // 2] = amplitude
        amp[1, y0:y0 + h, x0 + w // 2:x0 + w] = amplitude
    elif kind == 'same':
        amp[0, y0:y0 + h, x0:x0 + w] = amplitude
    elif kind == 'gauss':
        yy, xx = np.mgrid[:H, :W]
        prof = np.exp(-(((yy - (y0 + (h - 1) / 2.0)) / (h / 2.0)) ** 2 + ((xx - (x0 + (w - 1) / 2.0)) / (w / 2.0)) ** 2))
        amp[0, y0:y0 + h, x0:x0 + w] = amplitude * prof[y0:y0 + h, x0:x0 + w]
    f = f + s1[:, None, None] * amp[0][None] + s2[:, None, None] * amp[1][None] + sigma * rs.standard_normal((T, H, W))
    frames = np.rint(f).astype(np.int16)
    region = np.array([[y, x] for y in range(y0, y0 + h) for x in range(x0, x0 + w)], np.int64)
    left = region[region[:, 1] < x0 + w // 2]
    right = region[region[:, 1] >= x0 + w // 2]
    return frames, region, left, right, (n1, n2)


def corrcoef(frames, pix):
    """np.corrcoef of the pixels' series, float64; a constant pixel: 0 in its row and column."""
    x = frames[:, pix[:, 0], pix[:, 1]].astype(np.float64).T
    with np.errstate(invalid='ignore', divide='ignore'):
        c = np.corrcoef(x)
    return np.nan_to_num(np.atleast_2d(c), nan=0.0)


GPU_ORDER = ('static', 'two', 'same', 'gauss')       # the regions of gpu_scene, left to right
GPU_SEEDS = dict(static=0, two=2, same=0, gauss=0)   # tests/test_roi_pairs_api.py checks the reference gap of 'two': >= 0.15


def gpu_scene():
    """(10, 64) int16, T = 256: the four scenes side by side, each in a 10 x 16 frame of its own, and a strip of 9 pixels (below
    2 * min_area) in the top row.  -> frames, ROIs [static, two, strip, same, gauss] as (k,2) arrays, the two planted halves."""
    parts = [scene(kind, GPU_SEEDS[kind]) for kind in GPU_ORDER]
    frames = np.ascontiguousarray(np.concatenate([p[0] for p in parts], axis=2))
    regions = [p[1] + np.array([0, 16 * n]) for n, p in enumerate(parts)]
    strip = np.array([[0, x] for x in range(20, 29)], np.int64)
    rois = [regions[0], regions[1], strip, regions[2], regions[3]]
    return frames, rois, parts[1][2] + np.array([0, 16]), parts[1][3] + np.array([0, 16])
