"""Weighted ROI traces restated for the tests (include/dcunet.h, "Weighted ROI traces"; deep_calcium_amd/weighted.py): the weighted
sums entry by entry in Python integers, the weights of a footprint map, the exclusion of shared pixels, the Gram matrix and the
demix in exact rationals, all as plain loops, and the two-cell scene of the reach table.  Shares no code with the product."""
import math
from fractions import Fraction

import numpy as np

import _pair_ref as pref


# ---- the sums ----------------------------------------------------------------------------------------------------------------
def csr_sums(frames, row_off, row_pix, row_wgt, row_roi, R):
    """R rows of T Python ints: what dc_roi_wtrace_accumulate writes for the chunk `frames` (T,H,W).  An index outside the image
    adds nothing, a row whose ROI is outside [0, R) adds nowhere, a duplicate counts once per listing."""
    T = frames.shape[0]
    x = frames.reshape(T, -1)
    n = x.shape[1]
    out = [[0] * T for _ in range(R)]
    for s in range(len(row_off) - 1):
        r = s if row_roi is None else int(row_roi[s])
        if not 0 <= r < R:
            continue
        for e in range(int(row_off[s]), int(row_off[s + 1])):
            p, w = int(row_pix[e]), int(row_wgt[e])
            if not 0 <= p < n:
                continue
            for t in range(T):
                out[r][t] += w * int(x[t, p])
    return out


def roi_sums(frames, rois, weights):
    """(R,T) int64: sum of w x over each ROI's (y, x) entries; weights None: 1."""
    T, H, W = frames.shape
    out = []
    for r, c in enumerate(rois):
        row = [0] * T
        for e, (y, x) in enumerate(np.asarray(c).tolist()):
            w = 1 if weights is None else int(weights[r][e])
            for t in range(T):
                row[t] += w * int(frames[t, y, x])
        out.append(row)
    return np.array(out, np.int64)


def weight_sums(weights):
    return [sum(int(v) for v in w) for w in weights]


# ---- the host rules ----------------------------------------------------------------------------------------------------------
def weight_of(corr):
    """floor(256 max(corr, 0) + 0.5), NaN -> 0, at most 256."""
    c = float(corr)
    if c != c or c <= 0.0:
        return 0
    return min(256, int(math.floor(256.0 * c + 0.5)))


def footprint_weights(coords, corr, inside=None, floor=0.0):
    rois, weights, kept = [], [], []
    for r in range(len(coords)):
        cs, ws = [], []
        for e, yx in enumerate(np.asarray(coords[r]).tolist()):
            c = float(corr[r][e])
            if inside is not None and not bool(inside[r][e]):
                continue
            if c < floor or weight_of(c) == 0:
                continue
            cs.append(yx)
            ws.append(weight_of(c))
        if cs:
            rois.append(cs)
            weights.append(ws)
            kept.append(r)
    return rois, weights, kept


def exclude_overlap(rois, weights=None):
    """Pixels listed by more than one ROI are dropped; survivors in (y, x) order."""
    listed = {}
    for c in rois:
        for y, x in np.asarray(c).tolist():
            listed[(y, x)] = listed.get((y, x), 0) + 1
    out_r, out_w, kept = [], [], []
    for r, c in enumerate(rois):
        ent = sorted(((y, x), 1 if weights is None else int(weights[r][e])) for e, (y, x) in enumerate(np.asarray(c).tolist())
                     if listed[(y, x)] == 1)
        if ent:
            out_r.append([list(p) for p, _ in ent])
            out_w.append([w for _, w in ent])
            kept.append(r)
    return out_r, out_w, kept


def gram(rois, weights=None):
    """R x R Python ints: sum over shared pixels of w_i w_j, by the definition (every pair of ROIs, every pair of entries)."""
    R = len(rois)
    maps = []
    for r, c in enumerate(rois):
        maps.append(dict(((y, x), 1 if weights is None else int(weights[r][e])) for e, (y, x) in enumerate(np.asarray(c).tolist())))
    return [[sum(w * maps[j][p] for p, w in maps[i].items() if p in maps[j]) for j in range(R)] for i in range(R)]


def components(G):
    R = len(G)
    seen, out = set(), []
    for r in range(R):
        if r in seen:
            continue
        comp, todo = [], [r]
        seen.add(r)
        while todo:
            a = todo.pop()
            comp.append(a)
            for b in range(R):
                if b not in seen and G[a][b] != 0:
                    seen.add(b)
                    todo.append(b)
        out.append(sorted(comp))
    return out


def solve_exact(G, S):
    """G c = S over the rationals (Gauss-Jordan on Fractions); None where G is singular.  G: n x n ints, S: n x T ints."""
    n = len(G)
    m = [[Fraction(int(v)) for v in G[i]] + [Fraction(int(v)) for v in S[i]] for i in range(n)]
    for k in range(n):
        piv = next((i for i in range(k, n) if m[i][k] != 0), None)
        if piv is None:
            return None
        m[k], m[piv] = m[piv], m[k]
        d = m[k][k]
        m[k] = [v / d for v in m[k]]
        for i in range(n):
            if i != k and m[i][k] != 0:
                f = m[i][k]
                m[i] = [a - f * b for a, b in zip(m[i], m[k])]
    return [row[n:] for row in m]


def demix(sums, G):
    """(R,T) float64: the exact rational solution per component, each value rounded once.  ValueError for a singular component."""
    sums = np.asarray(sums)
    out = np.empty(sums.shape, np.float64)
    for comp in components(G):
        sol = solve_exact([[G[i][j] for j in comp] for i in comp], [sums[i].tolist() for i in comp])
        if sol is None:
            raise ValueError('singular component %s' % comp)
        for i, row in zip(comp, sol):
            out[i] = [float(v) for v in row]
    return out


# ---- the scene of the reach table ----------------------------------------------------------------------------------------------
SHAPE, T_REACH, CENTRES, RADIUS, CUT = (12, 20), 1024, (7.0, 12.0), 3.2, 0.2


def profiles():
    yy, xx = np.mgrid[:SHAPE[0], :SHAPE[1]]
    return [np.exp(-((yy - 5.5) / RADIUS) ** 2 - ((xx - cx) / RADIUS) ** 2) for cx in CENTRES]


def scene(seed, amplitude=60.0, sigma=30.0, T=T_REACH):
    """-> frames (T,12,20) int16, the two ROIs as (k,2) [y,x] (profile > 0.2, raster order), the two true activities."""
    rs = np.random.RandomState(7000 + seed)
    (s1, _), (s2, _), (npil, _) = pref._activity(rs, T), pref._activity(rs, T), pref._activity(rs, T)
    prof = profiles()
    f = 400.0 + 0.3 * amplitude * npil[:, None, None] * np.ones((1,) + SHAPE)
    f = f + s1[:, None, None] * (amplitude * prof[0])[None] + s2[:, None, None] * (amplitude * prof[1])[None]
    f = f + sigma * rs.standard_normal((T,) + SHAPE)
    rois = [np.argwhere(p > CUT).astype(np.int64) for p in prof]
    return np.rint(f).astype(np.int16), rois, (s1, s2)


def inside_corr(frames, roi):
    """corr(x_p, S - x_p) of every pixel of the ROI with the ROI's binary trace, the pixel's own series taken out: the exact integer
    numerators (int64 holds them here: T = 1024, |x| < 2^15, |S| < 2^22), each quotient in float64."""
    T = frames.shape[0]
    x = frames[:, roi[:, 0], roi[:, 1]].astype(np.int64)              # (T, k)
    S = x.sum(1)
    u, w = int(S.sum()), int((S * S).sum())
    out = []
    for e in range(x.shape[1]):
        a, b, c = int(x[:, e].sum()), int((x[:, e] * x[:, e]).sum()), int((x[:, e] * S).sum())
        cxx, cxs, css = T * b - a * a, T * c - a * u, T * w - u * u
        cxl, cll = cxs - cxx, css - 2 * cxs + cxx
        out.append(0.0 if cxx <= 0 or cll <= 0 else float(cxl) / (math.sqrt(float(cxx)) * math.sqrt(float(cll))))
    return np.array(out, np.float64)


def pearson(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / math.sqrt(float((a * a).sum()) * float((b * b).sum())))
