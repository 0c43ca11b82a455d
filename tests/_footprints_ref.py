"""The ROI footprint maps restated for the tests (include/dcunet.h, "ROI footprint maps"): moments and numerators in Python
integers, corr by the formula with float(int) (correctly rounded, like dc_i128_to_f64) and math.sqrt, an independent 60-digit
decimal evaluation of the exact quotient, and roi_support / refine_rois naively, pixel by pixel.  Shares no code with the product."""
import decimal
import math

import numpy as np


# ---- support ---------------------------------------------------------------------------------------------------------------
def support(pixel_sets, shape, halo):
    """pixel_sets: per ROI an iterable of (y, x).  -> (coords, inside) by brute force: every pixel of the image is tested against
    every pixel of the ROI."""
    H, W = shape
    coords, inside = [], []
    for pix in pixel_sets:
        own = set((int(y), int(x)) for y, x in pix)
        c, i = [], []
        for y in range(H):
            for x in range(W):
                if (y, x) in own:
                    c.append((y, x)); i.append(True)
                elif any(max(abs(y - py), abs(x - px)) <= halo for py, px in own):
                    c.append((y, x)); i.append(False)
        coords.append(np.array(c, np.int64).reshape(-1, 2))
        inside.append(np.array(i, bool))
    return coords, inside


# ---- moments and corr ------------------------------------------------------------------------------------------------------
def sums(frames, own_flat):
    """S_r(t) as Python ints: frames (T, H, W), own_flat the ROI's flat indices (outside the image: nothing)."""
    T = frames.shape[0]
    x = frames.reshape(T, -1)
    n = x.shape[1]
    return [sum(int(x[t, p]) for p in own_flat if 0 <= p < n) for t in range(T)]


def moments(frames, entries_flat, S):
    """Per entry (a, b, c) as Python ints; S the ROI's trace (Python ints).  An entry outside the image: (0, 0, 0)."""
    T = frames.shape[0]
    x = frames.reshape(T, -1)
    n = x.shape[1]
    out = []
    for p in entries_flat:
        if not 0 <= p < n:
            out.append((0, 0, 0))
            continue
        col = [int(v) for v in x[:, p]]
        out.append((sum(col), sum(v * v for v in col), sum(v * s for v, s in zip(col, S))))
    return out


def numerators(T, a, b, c, u, w, inside):
    cxx, cxs, css = T * b - a * a, T * c - a * u, T * w - u * u
    if inside:
        return cxx, cxs - cxx, css - 2 * cxs + cxx
    return cxx, cxs, css


def corr64(T, a, b, c, u, w, inside):
    """The contract's formula in doubles, before the rounding to float32."""
    cxx, cxl, cll = numerators(T, a, b, c, u, w, inside)
    if cxx <= 0 or cll <= 0:
        return 0.0
    return float(cxl) / (math.sqrt(float(cxx)) * math.sqrt(float(cll)))


def corr(T, a, b, c, u, w, inside):
    return np.float32(corr64(T, a, b, c, u, w, inside))


_CTX = decimal.Context(prec=60)


def corr_exact(T, a, b, c, u, w, inside):
    """Cxl / sqrt(Cxx Cll) in 60-digit decimal arithmetic, rounded once (decimal -> double -> float32; the double step moves the
    result by < 2^-29 float32 ulp)."""
    cxx, cxl, cll = numerators(T, a, b, c, u, w, inside)
    if cxx <= 0 or cll <= 0:
        return np.float32(0)
    return np.float32(float(_CTX.divide(decimal.Decimal(cxl), _CTX.sqrt(decimal.Decimal(cxx * cll)))))


def maps(frames, coords, inside, own_pixels):
    """Per ROI (moments list, corr float32 array, corr_exact float32 array).  coords: (k,2) [y,x] per ROI; own_pixels: per ROI its
    own (k,2) [y,x]."""
    T, H, W = frames.shape
    out = []
    for c, ins, own in zip(coords, inside, own_pixels):
        S = sums(frames, [int(y) * W + int(x) for y, x in own])
        u, w = sum(S), sum(s * s for s in S)
        mom = moments(frames, [int(y) * W + int(x) for y, x in c], S)
        out.append((mom,
                    np.array([corr(T, a, b, cc, u, w, bool(i)) for (a, b, cc), i in zip(mom, ins)], np.float32),
                    np.array([corr_exact(T, a, b, cc, u, w, bool(i)) for (a, b, cc), i in zip(mom, ins)], np.float32)))
    return out


# ---- refinement ------------------------------------------------------------------------------------------------------------
def refine(coords, corrs, shape, threshold, min_area=1):
    """Keep corr >= threshold, then the largest 8-connected component (flood fill; ties: the one with the smallest flat index),
    drop below min_area."""
    H, W = shape
    new, kept = [], []
    for r, (c, v) in enumerate(zip(coords, corrs)):
        left = set((int(y), int(x)) for (y, x), val in zip(c, v) if float(val) >= threshold)
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
        if not comps:
            continue
        best = max(comps, key=lambda g: (len(g), -(g[0][0] * W + g[0][1])))
        if len(best) < min_area:
            continue
        new.append(np.array(best, np.int64).reshape(-1, 2))
        kept.append(r)
    return new, kept


# ---- the synthetic scene of the tests -----------------------------------------------------------------------------------------
def scene():
    """(24, 24), T = 400, int16: one active cell (pixel weights times a sparse activity plus independent noise), one static bright
    blob (noise only), and a mask that covers both, each dilated by one pixel.
    -> frames, mask ROIs [cell + ring, blob + ring] as (k,2) arrays, the true cell's (k,2) pixels, the blob's."""
    rs = np.random.RandomState(11)
    T, H, W = 400, 24, 24
    frames = 200 + rs.randint(-20, 21, size=(T, H, W))
    yy, xx = np.mgrid[:H, :W]
    cell = (yy - 6) ** 2 + (xx - 7) ** 2 <= 6
    blob = (yy - 16) ** 2 + (xx - 16) ** 2 <= 6
    activity = np.zeros(T, np.int64)
    onsets = rs.choice(T - 10, 25, replace=False)
    for o in onsets:
        activity[o:o + 6] += (np.array([10, 8, 6, 4, 2, 1]) * rs.randint(1, 4)).astype(np.int64)
    weight = rs.randint(8, 13, size=(H, W)) * cell
    frames = frames + activity[:, None, None] * weight[None]
    frames = frames + 600 * blob[None]                       # bright, but it never fires
    assert frames.min() >= 0 and frames.max() < 32768
    frames = frames.astype(np.int16)

    def grow(m):
        g = m.copy()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                g[max(0, dy):H + min(0, dy), max(0, dx):W + min(0, dx)] |= m[max(0, -dy):H + min(0, -dy), max(0, -dx):W + min(0, -dx)]
        return g
    rois = [np.argwhere(grow(cell)), np.argwhere(grow(blob))]
    return frames, rois, np.argwhere(cell), np.argwhere(blob)
