"""The numpy oracle of piecewise-rigid motion correction: a plain int64 restatement of the definitions in include/dcunet.h (block
geometry, block scores, block pick, shift field, warp).  Everything is exact; a shift (dy, dx) means out[y, x] = frame[y + dy, x + dx]."""
import numpy as np


def edges(n, B):
    """e(i) = floor(i * n / B), i = 0 .. B."""
    return [i * n // B for i in range(B + 1)]


def clipped(n, B, M):
    """[(lo, hi)] of every block clipped to the interior [M, n - M)."""
    e = edges(n, B)
    return [(max(e[i], M), min(e[i + 1], n - M)) for i in range(B)]


def grid_ok(H, W, By, Bx, M):
    return all(lo < hi for n, B in ((H, By), (W, Bx)) for lo, hi in clipped(n, B, M))


def clamp_rigid(rigid, S):
    return np.clip(np.asarray(rigid, np.int64), -S, S)


def block_scores(frames, tmpl, S, D, By, Bx, rigid):
    """(t, By, Bx, 2D+1, 2D+1) int64: the sum over the clipped block of (tmpl[y, x] - f[y + dy + ey, x + dx + ex])^2, (dy, dx) the
    frame's rigid shift clamped to [-S, S]."""
    frames, tmpl = np.asarray(frames), np.asarray(tmpl)
    T, H, W = frames.shape
    M = S + D
    assert grid_ok(H, W, By, Bx, M)
    r = clamp_rigid(rigid, S)
    t64, f64 = tmpl.astype(np.int64), frames.astype(np.int64)
    out = np.zeros((T, By, Bx, 2 * D + 1, 2 * D + 1), np.int64)
    for t in range(T):
        dy, dx = int(r[t, 0]), int(r[t, 1])
        for i, (y0, y1) in enumerate(clipped(H, By, M)):
            for j, (x0, x1) in enumerate(clipped(W, Bx, M)):
                for ey in range(-D, D + 1):
                    for ex in range(-D, D + 1):
                        d = t64[y0:y1, x0:x1] - f64[t, y0 + dy + ey:y1 + dy + ey, x0 + dx + ex:x1 + dx + ex]
                        out[t, i, j, ey + D, ex + D] = (d * d).sum()
    return out


def block_pick(bsc, rigid, S):
    """(t, By, Bx, 2) int32 block shifts and (t, By, Bx) int64 best scores: the residual minimises (score, ey^2 + ex^2, ey, ex)."""
    bsc = np.asarray(bsc)
    T, By, Bx, nd = bsc.shape[:4]
    D = (nd - 1) // 2
    r = clamp_rigid(rigid, S)
    out = np.zeros((T, By, Bx, 2), np.int32)
    best = np.zeros((T, By, Bx), np.int64)
    for t in range(T):
        for i in range(By):
            for j in range(Bx):
                sc, _, ey, ex = min((int(bsc[t, i, j, ey + D, ex + D]), ey * ey + ex * ex, ey, ex)
                                    for ey in range(-D, D + 1) for ex in range(-D, D + 1))
                out[t, i, j] = (r[t, 0] + ey, r[t, 1] + ex)
                best[t, i, j] = sc
    return out, best


def taps(n, B):
    """[(i0, i1, w)] for every pixel of an axis of n pixels in B blocks, in doubled coordinates."""
    e = edges(n, B)
    c2 = [e[i] + e[i + 1] - 1 for i in range(B)]
    out = []
    for y in range(n):
        p = 2 * y
        if B == 1 or p <= c2[0]:
            out.append((0, 0, 0))
        elif p >= c2[B - 1]:
            out.append((B - 1, B - 1, 0))
        else:
            i0 = max(i for i in range(B) if c2[i] <= p)
            out.append((i0, i0 + 1, 256 * (p - c2[i0]) // (c2[i0 + 1] - c2[i0])))
    return out


def field(bs, H, W):
    """(H, W, 2) int64: the shift field of one frame's block shifts bs (By, Bx, 2) as nested lists of python ints -- the arithmetic
    is python's, so it is exact for any int32, and the result lies within the block shifts."""
    By, Bx = len(bs), len(bs[0])
    rows, cols = taps(H, By), taps(W, Bx)
    out = np.zeros((H, W, 2), np.int64)
    for y, (i0, i1, w) in enumerate(rows):
        for x, (j0, j1, v) in enumerate(cols):
            for c in range(2):
                s00, s01, s10, s11 = (int(bs[i0][j0][c]), int(bs[i0][j1][c]), int(bs[i1][j0][c]), int(bs[i1][j1][c]))
                num = (256 - w) * ((256 - v) * s00 + v * s01) + w * ((256 - v) * s10 + v * s11)
                out[y, x, c] = (num + 32768) // 65536          # python ints: floor division, no overflow
    return out


def warp(frames, bshifts, fill=0):
    """out[t, y, x] = frames[t, y + fy, x + fx] inside the frame, fill elsewhere."""
    frames = np.asarray(frames)
    T, H, W = frames.shape
    out = np.full_like(frames, np.array(fill).astype(frames.dtype))
    yy, xx = np.mgrid[0:H, 0:W]
    for t in range(T):
        f = field(np.asarray(bshifts[t]).tolist(), H, W)
        sy, sx = yy + f[:, :, 0], xx + f[:, :, 1]
        ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
        out[t][ok] = frames[t][sy[ok], sx[ok]]
    return out
