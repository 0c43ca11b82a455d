"""The oracle of the dF/F tests: include/dcunet.h ("dF/F traces") restated in plain numpy int64, a sort per frame, and a
brute-force Chebyshev ring.  Nothing here is shared with deep_calcium_amd/dff.py."""
import numpy as np


def rank(q, n):
    return (q * (n - 1)) // 100


def baseline(num, half, q):
    """num (R, T) int64 -> B (R, T) int64: np.sort(window)[k] over [max(0, t - h), min(T - 1, t + h)]."""
    num = np.asarray(num, np.int64)
    R, T = num.shape
    out = np.empty((R, T), np.int64)
    for t in range(T):
        a, b = max(0, t - half), min(T - 1, t + half)
        w = np.sort(num[:, a:b + 1], axis=1)
        out[:, t] = w[:, rank(q, b - a + 1)]
    return out


def dff(num, base):
    """float32 (R, T): ((N - B) / B in float64).astype(float32) where B > 0, exactly 0 elsewhere."""
    num, base = np.asarray(num, np.int64), np.asarray(base, np.int64)
    safe = np.where(base > 0, base, 1)
    out = ((num - base).astype(np.float64) / safe.astype(np.float64)).astype(np.float32)
    return np.where(base > 0, out, np.float32(0)).astype(np.float32)


def scale(x, den):
    x, den = np.asarray(x, np.int64), np.asarray(den, np.int64)
    safe = np.where(den > 0, den, 1)
    out = (x.astype(np.float64) / safe.astype(np.float64)[:, None]).astype(np.float32)
    return np.where((den > 0)[:, None], out, np.float32(0)).astype(np.float32)


def weight_256ths(w):
    return int(np.floor(256.0 * w + 0.5))


def numerators(S, A, Sn=None, An=None, weight=0.7, offset=0):
    """-> (N (R, T) int64, D (R,) int64).  Sn / An: the ring sums and areas, row for row; An[r] == 0: no correction."""
    S, A = np.asarray(S, np.int64), np.asarray(A, np.int64)
    N = S + offset * A[:, None]
    D = A.copy()
    if Sn is not None:
        a = weight_256ths(weight)
        Sn, An = np.asarray(Sn, np.int64), np.asarray(An, np.int64)
        for r in range(len(A)):
            if An[r] > 0:
                N[r] = 256 * An[r] * (S[r] + offset * A[r]) - a * A[r] * (Sn[r] + offset * An[r])
                D[r] = 256 * An[r] * A[r]
    return N, D


def rings(rois, shape, inner, outer):
    """rois: list of (k, 2) [y, x] arrays.  Brute force: the Chebyshev distance of every pixel to every ROI."""
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    dist = []
    for c in rois:
        c = np.asarray(c).reshape(-1, 2)
        d = np.maximum(np.abs(yy[..., None] - c[:, 0]), np.abs(xx[..., None] - c[:, 1])).min(-1)
        dist.append(d)
    nearest = np.min(dist, axis=0)
    return [np.argwhere((d > inner) & (d <= outer) & (nearest > inner)).reshape(-1, 2) for d in dist]
