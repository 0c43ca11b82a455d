"""The oracle of the wide (coarse-to-fine) shift search: a numpy int64 / Python-int restatement of the six steps in
include/dcunet.h -- bin, coarse pick, centre, window scores, pick over total shifts, refinement -- built on _motion_ref.scores / pick
and _motion_sub_ref.refine_q.  Everything is exact; a shift (dy, dx) means out[y, x] = frame[y + dy, x + dx]."""
import numpy as np

import _motion_ref as ref
import _motion_sub_ref as sref

Q = sref.Q


def bin_frames(frames, c):
    """(..., H // c, W // c) of the frames' dtype: floor((sum of the c x c cell + c^2 / 2) / c^2); trailing rows and columns dropped."""
    frames = np.asarray(frames)
    H, W = frames.shape[-2:]
    Hc, Wc = H // c, W // c
    assert c in (2, 4, 8) and Hc > 0 and Wc > 0
    cells = frames[..., :Hc * c, :Wc * c].astype(np.int64).reshape(frames.shape[:-2] + (Hc, c, Wc, c))
    return ((cells.sum(axis=(-3, -1)) + c * c // 2) // (c * c)).astype(frames.dtype)        # // floors for either sign


def centres(rows, mult, S, D):
    """(t, 2) int64: clamp(mult * rows, -(S - D), S - D) per component, the product in Python integers."""
    M = S - D
    assert M >= 0
    return np.array([[max(-M, min(M, int(mult) * int(v))) for v in row] for row in np.asarray(rows).reshape(-1, 2)], np.int64).reshape(-1, 2)


def window_scores(frames, tmpl, S, D, rows, mult):
    """(t, 2D+1, 2D+1) int64: the sums over the radius-S interior at centre + (ey, ex)."""
    frames, tmpl = np.asarray(frames), np.asarray(tmpl)
    T, H, W = frames.shape
    assert 0 <= D <= S and H > 2 * S and W > 2 * S and tmpl.shape == (H, W)
    ctr = centres(rows, mult, S, D)
    t = tmpl[S:H - S, S:W - S].astype(np.int64)
    out = np.zeros((T, 2 * D + 1, 2 * D + 1), np.int64)
    for k in range(T):
        f = frames[k].astype(np.int64)
        for ey in range(-D, D + 1):
            for ex in range(-D, D + 1):
                dy, dx = int(ctr[k, 0]) + ey, int(ctr[k, 1]) + ex
                d = t - f[S + dy:H - S + dy, S + dx:W - S + dx]
                out[k, ey + D, ex + D] = (d * d).sum()
    return out


def pick_around(wscores, rows, mult, S):
    """(shifts (t, 2) int32, best (t,) int64, fine (t, 2) int32): the total shift centre + (ey, ex) minimising
    (score, dy^2 + dx^2, dy, dx), its score, and 16 * shift + q with q from the window table at the picked residual."""
    wscores = np.asarray(wscores)
    T, nd = wscores.shape[:2]
    D = (nd - 1) // 2
    ctr = centres(rows, mult, S, D)
    shifts, best, fine = np.zeros((T, 2), np.int32), np.zeros(T, np.int64), np.zeros((T, 2), np.int32)
    for k in range(T):
        cy, cx = int(ctr[k, 0]), int(ctr[k, 1])
        sc, _, dy, dx = min((int(wscores[k, ey + D, ex + D]), (cy + ey) ** 2 + (cx + ex) ** 2, cy + ey, cx + ex)
                            for ey in range(-D, D + 1) for ex in range(-D, D + 1))
        qy, qx = sref.refine_entry(wscores[k], dy - cy, dx - cx)
        shifts[k], best[k], fine[k] = (dy, dx), sc, (Q * dy + qy, Q * dx + qx)
    return shifts, best, fine


def search(frames, tmpl, S, c):
    """The whole wide search -> dict(coarse, cscores, wscores, shifts, best, fine)."""
    Sc = -(-S // c)
    bf, bt = bin_frames(frames, c), bin_frames(tmpl, c)
    cscores = ref.scores(bf, bt, Sc)
    coarse = ref.pick(cscores)
    wscores = window_scores(frames, tmpl, S, c, coarse, c)
    shifts, best, fine = pick_around(wscores, coarse, c, S)
    return dict(coarse=coarse, cscores=cscores, wscores=wscores, shifts=shifts, best=best, fine=fine)


def planted(H, W, S, c, dtype):
    """The end-to-end dataset of the tests: a uniform-random 16-bit scene (H + 2S, W + 2S) from RandomState(H + S + c), the four
    corners (+-S, +-S), (0, 0), (S, -1), (-1, 0) and 25 random offsets in [-S, S] from the same stream -> (template, frames,
    offsets)."""
    rs = np.random.RandomState(H + S + c)
    info = np.iinfo(dtype)
    scene = rs.randint(info.min, info.max + 1, size=(H + 2 * S, W + 2 * S)).astype(dtype)
    offsets = [(S, S), (S, -S), (-S, S), (-S, -S), (0, 0), (S, -1), (-1, 0)] + [tuple(int(v) for v in rs.randint(-S, S + 1, size=2)) for _ in range(25)]
    tmpl, frames = ref.cut(scene, H, W, S, offsets)
    return tmpl, frames, np.array(offsets, np.int64)
