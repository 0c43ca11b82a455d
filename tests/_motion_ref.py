"""The numpy oracle of rigid motion correction: a plain int64 restatement of the three definitions (score, shift, correction),
the valid rectangle and the rounded-mean template.  Everything is exact; a shift (dy, dx) means out[y, x] = frame[y + dy, x + dx]."""
import numpy as np


def scores(frames, tmpl, S):
    """(t, 2S+1, 2S+1) int64: score[dy+S, dx+S] = sum over y in [S, H-S), x in [S, W-S) of (tmpl[y, x] - f[y+dy, x+dx])^2."""
    frames, tmpl = np.asarray(frames), np.asarray(tmpl)
    T, H, W = frames.shape
    assert 0 <= S and H > 2 * S and W > 2 * S and tmpl.shape == (H, W)
    t = tmpl[S:H - S, S:W - S].astype(np.int64)
    f = frames.astype(np.int64)
    out = np.zeros((T, 2 * S + 1, 2 * S + 1), np.int64)
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            d = t[None] - f[:, S + dy:H - S + dy, S + dx:W - S + dx]
            out[:, dy + S, dx + S] = (d * d).sum(axis=(1, 2))
    return out


def pick(sc):
    """(t, 2) int32: the (dy, dx) that minimises the tuple (score, dy^2 + dx^2, dy, dx) lexicographically."""
    sc = np.asarray(sc)
    T, nd = sc.shape[0], sc.shape[1]
    S = (nd - 1) // 2
    out = np.zeros((T, 2), np.int32)
    for t in range(T):
        out[t] = min((int(sc[t, dy + S, dx + S]), dy * dy + dx * dx, dy, dx)
                     for dy in range(-S, S + 1) for dx in range(-S, S + 1))[2:]
    return out


def apply(frames, shifts, fill=0):
    """out[t, y, x] = frames[t, y + dy, x + dx] inside the frame, fill elsewhere; any integer shift."""
    frames = np.asarray(frames)
    T, H, W = frames.shape
    out = np.full_like(frames, np.array(fill).astype(frames.dtype))
    for t in range(T):
        dy, dx = int(shifts[t][0]), int(shifts[t][1])
        y0, y1 = max(0, -dy), min(H, H - dy)
        x0, x1 = max(0, -dx), min(W, W - dx)
        if y0 < y1 and x0 < x1:
            out[t, y0:y1, x0:x1] = frames[t, y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return out


def valid(shifts, shape):
    H, W = shape
    s = np.asarray(shifts, np.int64).reshape(-1, 2)
    return ((max(0, -int(s[:, 0].min())), H - max(0, int(s[:, 0].max()))),
            (max(0, -int(s[:, 1].min())), W - max(0, int(s[:, 1].max()))))


def rounded_mean(frames):
    """floor((2 * sum + N) / (2 N)) per pixel, in the frames' dtype."""
    frames = np.asarray(frames)
    N = frames.shape[0]
    total = frames.astype(np.int64).sum(0)
    return ((2 * total + N) // (2 * N)).astype(frames.dtype)


def make_template(frames, S, iterations=1):
    tmpl = rounded_mean(frames)
    for _ in range(iterations):
        tmpl = rounded_mean(apply(frames, pick(scores(frames, tmpl, S)), 0))
    return tmpl


def cut(scene, H, W, S, offsets):
    """Frames cut from `scene` (H + 2S, W + 2S) at offsets (a, b) relative to the central crop; -> (template, frames)."""
    tmpl = scene[S:S + H, S:S + W].copy()
    frames = np.stack([scene[S + a:S + a + H, S + b:S + b + W] for a, b in offsets])
    return tmpl, frames
