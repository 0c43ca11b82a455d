"""The detrended (segment-pooled) correlations restated for the tests (include/dcunet.h, "Detrended correlations"): the segment
plan, per-segment moments and pooled numerators in exact integers, corr as the exact quotient in 60-digit decimal arithmetic
rounded once (the formula of _pair_ref.corr_exact), std likewise, and the bleaching of the scenes.  numpy / Python integers only;
shares no code with the product."""
import decimal
import math

import numpy as np

MAX_FRAMES = 4096
_CTX = decimal.Context(prec=60)
_D = decimal.Decimal


# ---- the plan --------------------------------------------------------------------------------------------------------------
def plan(T, L):
    """-> [(t_start, len, mult)] by the words of the header: n = max(1, T // L) segments, the last absorbs the remainder."""
    n = max(1, T // L)
    if n == 1:
        return [(0, T, 1)]
    last = T - (n - 1) * L
    segs = []
    for s in range(n):
        length = L if s < n - 1 else last
        segs.append((s * L, length, (L * last) // length))
    return segs


def big_m(T, L):
    segs = plan(T, L)
    return segs[0][1] * segs[0][2]


def bleach(frames, beta):
    """floor(frame_t * exp(ln(beta) * t / (T - 1)) + 0.5) as int16: the recording decays to the fraction beta of its start."""
    T = frames.shape[0]
    decay = np.exp(math.log(beta) * np.arange(T) / (T - 1.0))
    return np.floor(frames.astype(np.float64) * decay[:, None, None] + 0.5).astype(np.int16)


# ---- pooled numerators --------------------------------------------------------------------------------------------------------
def _exact(X):
    """(T, k) integers -> an array that multiplies exactly: int64 where every pooled numerator provably fits, Python ints else."""
    X = np.asarray(X)
    top = int(np.abs(X.astype(np.int64)).max()) if X.size else 0
    if top * top * X.shape[0] * 2 ** 26 < 2 ** 62:      # |N| <= top^2 T M and M < 2^25 (or M = T)
        return X.astype(np.int64)
    return X.astype(object)


def pooled_pair(x, y, L):
    """Two series as sequences of ints -> N(x, y), by the definition, in Python integers."""
    x, y = [int(v) for v in x], [int(v) for v in y]
    total = 0
    for t0, length, mult in plan(len(x), L):
        xs, ys = x[t0:t0 + length], y[t0:t0 + length]
        total += mult * (length * sum(a * b for a, b in zip(xs, ys)) - sum(xs) * sum(ys))
    return total


def pooled_gram(X, L):
    """X (T, k) -> the (k, k) matrix of N(x_i, x_j), an object array of Python ints (symmetric)."""
    X = _exact(X)
    T, k = X.shape
    N = np.zeros((k, k), X.dtype)
    for t0, length, mult in plan(T, L):
        S = X[t0:t0 + length]
        a = S.sum(0)
        N = N + mult * (length * S.T.dot(S) - np.outer(a, a))
    return N.astype(object)


def pooled_cross(X, Y, L):
    """X (T, k), Y (T, m) -> (k, m) of N(x_i, y_j)."""
    both = _exact(np.concatenate([np.asarray(X).astype(object), np.asarray(Y).astype(object)], 1))
    X, Y = both[:, :X.shape[1]], both[:, X.shape[1]:]
    N = np.zeros((X.shape[1], Y.shape[1]), both.dtype)
    for t0, length, mult in plan(X.shape[0], L):
        A, B = X[t0:t0 + length], Y[t0:t0 + length]
        N = N + mult * (length * A.T.dot(B) - np.outer(A.sum(0), B.sum(0)))
    return N.astype(object)


# ---- one-rounding quotients -----------------------------------------------------------------------------------------------------
def _quot(nxy, nxx, nyy):
    return _CTX.divide(_D(int(nxy)), _CTX.sqrt(_D(int(nxx) * int(nyy))))


def corr_exact(nxx, nxy, nyy):
    """N(x,y) / sqrt(N(x,x) N(y,y)) in 60-digit decimal arithmetic, rounded once; 0 where a numerator of the denominator is <= 0."""
    if nxx <= 0 or nyy <= 0:
        return np.float32(0)
    return np.float32(float(_quot(nxy, nxx, nyy)))


def std_exact(nxx, M, T):
    return np.float32(float(_CTX.sqrt(_CTX.divide(_D(int(nxx)), _D(M * T)))))


def pair_corr(N):
    k = len(N)
    return np.array([[corr_exact(N[i][i], N[i][j], N[j][j]) for j in range(k)] for i in range(k)], np.float32).reshape(k, k)


# ---- the series image -----------------------------------------------------------------------------------------------------------
SLOTS = ((0, 1), (1, 0), (1, 1), (1, -1))             # right, down, down-right, down-left: the pair is stored with the EARLIER pixel


def series_numerators(frames, L):
    """-> (var (H,W), cov (4,H,W)) object arrays of Python ints; cov[j][y][x] = N(pixel, its neighbour j), 0 where it is outside."""
    T, H, W = frames.shape
    F = np.asarray(frames).astype(object)               # Python ints: every product and sum below is exact
    var = np.zeros((H, W), object)
    cov = np.zeros((4, H, W), object)
    for t0, length, mult in plan(T, L):
        S = F[t0:t0 + length]
        a = S.sum(0)
        var = var + mult * (length * (S * S).sum(0) - a * a)
        for j, (dy, dx) in enumerate(SLOTS):
            # the pixels (y, x) whose neighbour (y + dy, x + dx) is inside the image, and those neighbours
            ys, xs = slice(0, H - dy), slice(max(0, -dx), W - max(0, dx))
            yq, xq = slice(dy, H), slice(max(0, dx), W + min(0, dx))
            if S[:, ys, xs].size:
                cov[j, ys, xs] = cov[j, ys, xs] + mult * (length * (S[:, ys, xs] * S[:, yq, xq]).sum(0) - a[ys, xs] * a[yq, xq])
    return var, cov


def series_corr(var, cov):
    """The mean over the neighbours inside the image of the exact quotients (a pair with a non-positive N(x,x) counts 0), rounded
    once to float32."""
    H, W = var.shape
    out = np.zeros((H, W), np.float32)
    for y in range(H):
        for x in range(W):
            acc, cnt = _D(0), 0
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    qy, qx = y + dy, x + dx
                    if (dy == 0 and dx == 0) or not (0 <= qy < H and 0 <= qx < W):
                        continue
                    cnt += 1
                    if var[y, x] <= 0 or var[qy, qx] <= 0:
                        continue
                    earlier = (y, x, dy, dx) if (dy, dx) > (0, 0) else (qy, qx, -dy, -dx)
                    n = cov[SLOTS.index(earlier[2:]), earlier[0], earlier[1]]
                    acc = _CTX.add(acc, _quot(n, var[y, x], var[qy, qx]))
            out[y, x] = np.float32(float(_CTX.divide(acc, _D(cnt)))) if cnt else np.float32(0)
    return out


def series_std(var, M, T):
    return np.array([[std_exact(v, M, T) for v in row] for row in var], np.float32).reshape(var.shape)


# ---- footprints -------------------------------------------------------------------------------------------------------------------
def footprint_numerators(frames, own, support, L):
    """own / support: flat pixel indices of the ROI and of its support -> (Cxx list, Cxs list, Css) of Python ints: the pooled
    numerators of every support pixel with itself and with the ROI's trace S, and of S with itself."""
    T = frames.shape[0]
    flat = frames.reshape(T, -1).astype(np.int64)
    S = flat[:, list(own)].sum(1)[:, None]
    X = flat[:, list(support)]
    cxs = pooled_cross(X, S, L)[:, 0]
    css = pooled_gram(S, L)[0][0]
    X = _exact(X)
    cxx = np.zeros(X.shape[1], X.dtype)
    for t0, length, mult in plan(T, L):
        A = X[t0:t0 + length]
        cxx = cxx + mult * (length * (A * A).sum(0) - A.sum(0) ** 2)
    return [int(v) for v in cxx], [int(v) for v in cxs], int(css)


def footprint_corr(cxx, cxs, css, inside):
    """The inside / halo rule on the pooled numerators, then the exact quotient rounded once."""
    out = []
    for xx, xs, ins in zip(cxx, cxs, inside):
        xl, ll = (xs - xx, css - 2 * xs + xx) if ins else (xs, css)
        out.append(corr_exact(xx, xl, ll))
    return np.array(out, np.float32)
