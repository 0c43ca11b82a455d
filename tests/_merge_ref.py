"""The ROI trace-pair correlation and the merge rule restated for the tests (include/dcunet.h, "ROI trace-pair correlation"): the
numerators of two rows in Python integers by the definition, corr as the exact quotient in 60-digit decimal arithmetic rounded
once, the 128-bit words, the neighbour list by brute force, the merge rule as a flood fill over plain lists, and the reach scenes.
Shares no code with the product."""
import numpy as np

import _detrend_ref as dref
import _pair_ref as pref


# ---- numerators and corr ------------------------------------------------------------------------------------------------------
def plan(T, L):
    """L: None or 0 -- one segment of T frames; otherwise _detrend_ref.plan."""
    return dref.plan(T, L) if L else [(0, T, 1)]


def big_m(T, L):
    segs = plan(T, L)
    return segs[0][1] * segs[0][2]


def pooled(x, y, L):
    """Two rows of ints -> N(x, y) = sum_s mult_s (L_s g_s - a_s a'_s), in Python integers."""
    x, y = [int(v) for v in x], [int(v) for v in y]
    total = 0
    for t0, length, mult in plan(len(x), L):
        xs, ys = x[t0:t0 + length], y[t0:t0 + length]
        total += mult * (length * sum(a * b for a, b in zip(xs, ys)) - sum(xs) * sum(ys))
    return total


def moments(sums, pairs, L):
    """sums: rows of ints; pairs: (i, j) -> [(Nxx, Nxy, Nyy)], zeros for a pair that names no row."""
    R = len(sums)
    out = []
    for i, j in pairs:
        if not (0 <= i < R and 0 <= j < R):
            out.append((0, 0, 0))
            continue
        out.append((pooled(sums[i], sums[i], L), pooled(sums[i], sums[j], L), pooled(sums[j], sums[j], L)))
    return out


def words(n):
    """A Python int -> (lo, hi) as int64 values, two's complement over 128 bits."""
    assert -(1 << 127) <= n < (1 << 127)
    u = n & ((1 << 128) - 1)
    lo, hi = u & ((1 << 64) - 1), u >> 64
    return (lo - (1 << 64) if lo >= (1 << 63) else lo), (hi - (1 << 64) if hi >= (1 << 63) else hi)


def moment_words(moms):
    return np.array([[w for n in m for w in words(n)] for m in moms], np.int64).reshape(-1, 6)


def corr(moms):
    """float32 (P,): N(x,y) / sqrt(N(x,x) N(y,y)) in 60-digit decimals, rounded once; 0 where N(x,x) <= 0 or N(y,y) <= 0."""
    return np.array([dref.corr_exact(nxx, nxy, nyy) for nxx, nxy, nyy in moms], np.float32).reshape(-1)


def corr64(moms):
    """The same quotients as float64 (for margins, never compared with the device)."""
    return np.array([float(dref._quot(nxy, nxx, nyy)) if nxx > 0 and nyy > 0 else 0.0 for nxx, nxy, nyy in moms], np.float64).reshape(-1)


# ---- neighbours and the merge rule ----------------------------------------------------------------------------------------------
def neighbours(rois, max_dist):
    """rois: lists of (y, x) -> [(i, j)], i < j, lexicographic: some pixel of i within Chebyshev distance max_dist of some pixel of j."""
    out = []
    for i in range(len(rois)):
        for j in range(i + 1, len(rois)):
            if any(max(abs(int(a[0]) - int(b[0])), abs(int(a[1]) - int(b[1]))) <= max_dist for a in rois[i] for b in rois[j]):
                out.append((i, j))
    return out


def merge(rois, pairs, corr, W, threshold):
    """rois: lists of (y, x) -> (new_rois as sorted lists of (y, x), origin): flood fill over the accepted pairs."""
    R = len(rois)
    adj = [set() for _ in range(R)]
    for (i, j), c in zip(pairs, corr):
        if float(c) >= threshold:
            adj[int(i)].add(int(j))
            adj[int(j)].add(int(i))
    seen, comps = set(), []
    for r in range(R):
        if r in seen:
            continue
        comp, todo = [], [r]
        seen.add(r)
        while todo:
            a = todo.pop()
            comp.append(a)
            for b in adj[a]:
                if b not in seen:
                    seen.add(b)
                    todo.append(b)
        comp.sort()
        flat = sorted(set(int(y) * W + int(x) for m in comp for y, x in rois[m]))
        comps.append((flat[0], comp[0], flat, comp))
    comps.sort(key=lambda c: (c[0], c[1]))
    return [[(f // W, f % W) for f in c[2]] for c in comps], [c[3] for c in comps]


# ---- the reach scenes ---------------------------------------------------------------------------------------------------------------
def half_sums(kind, seed, T=1024, beta=None, amplitude=60.0, sigma=30.0):
    """_pair_ref.scene, optionally bleached to the fraction beta -> the int sums of the left and of the right half over time."""
    frames, _, left, right, _ = pref.scene(kind, seed, amplitude, sigma, T=T)
    if beta is not None:
        frames = dref.bleach(frames, beta)
    f = frames.astype(np.int64)
    return f[:, left[:, 0], left[:, 1]].sum(1).tolist(), f[:, right[:, 0], right[:, 1]].sum(1).tolist()


def half_corr(kind, seed, L, T=1024, beta=None):
    x, y = half_sums(kind, seed, T, beta)
    return float(corr64(moments([x, y], [(0, 1)], L))[0])
