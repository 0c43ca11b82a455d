"""The numpy oracle of the bidirectional scan-phase correction (include/dcunet.h dc_bidi_scores / dc_bidi_apply and the host
pick), and the planted-offset recordings tests/test_bidi_api.py and tests/test_bidi_gpu.py share.  numpy only."""
import numpy as np


def scores(frames, P):
    """(t, 2P+1) int64: per frame and offset p the sum over odd y in [1, H-1), x in [P, W-P) of
    (2 f[y][x+p] - f[y-1][x] - f[y+1][x])^2."""
    f = np.asarray(frames).astype(np.int64)
    t, H, W = f.shape
    ys = np.arange(1, H - 1, 2)
    n = f[:, ys - 1, P:W - P] + f[:, ys + 1, P:W - P]
    out = np.zeros((t, 2 * P + 1), np.int64)
    for p in range(-P, P + 1):
        e = 2 * f[:, ys, P + p:W - P + p] - n
        out[:, p + P] = (e * e).reshape(t, -1).sum(axis=1)
    return out


def totals(sc):
    """The scores summed over the frames, as Python ints (object dtype underneath: no 64-bit wrap)."""
    return [int(v) for v in np.asarray(sc).astype(object).sum(axis=0)]


def pick(tot):
    """argmin of (total, p^2, p)."""
    P = len(tot) // 2
    return min(range(-P, P + 1), key=lambda p: (int(tot[p + P]), p * p, p))


def apply(frames, p, fill=0):
    """out[y][x] = frame[y][x + p] for odd y (fill outside the row), frame[y][x] for even y; fill: a 16-bit value as an int in
    [-32768, 65535], stored by its bits."""
    f = np.asarray(frames)
    out = f.copy()
    W = f.shape[-1]
    out[..., 1::2, :] = np.array([fill & 0xffff], np.uint16).view(f.dtype)[0]
    p = int(p)
    if abs(p) < W:
        lo, hi = max(0, -p), W - max(0, p)
        out[..., 1::2, lo:hi] = f[..., 1::2, lo + p:hi + p]
    return out


def valid_columns(xshifts, W, p, fine=False):
    """(x0, x1): the columns where the shift move AND the shift move of a line moved by p read inside the row; xshifts: the x
    shifts (fine: sixteenths; a used tap is floor and, off a whole pixel, floor + 1), or None for no registration."""
    xs = [0] if xshifts is None else [int(v) for v in np.asarray(xshifts).reshape(-1)]
    ok = np.ones(W, bool)
    x = np.arange(W)
    for s in xs:
        for q in (0, p):
            if fine and xshifts is not None:
                a, b = s // 16 + q, -((-s) // 16) + q
            else:
                a = b = s + q
            ok &= (x + a >= 0) & (x + b < W)
    idx = np.flatnonzero(ok)
    return (int(idx[0]), int(idx[-1]) + 1) if len(idx) else (0, 0)


# ---- planted recordings ---------------------------------------------------------------------------------------------------------------
def scene(rs, H, W, blobs, margin):
    """A float64 (H, W + 2 margin) scene: `blobs` Gaussian blobs (sigma 2.5 - 3, amplitude 150 - 300) on a baseline of 400."""
    yy, xx = np.mgrid[0:H, 0:W + 2 * margin].astype(np.float64)
    img = np.full((H, W + 2 * margin), 400.0)
    for _ in range(blobs):
        cy, cx = rs.uniform(0, H), rs.uniform(0, W + 2 * margin)
        sg, amp = rs.uniform(2.5, 3.0), rs.uniform(150.0, 300.0)
        img += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sg * sg))
    return img


def planted(seed, H, W, P, blobs, sigma, frames, b, dtype=np.int16):
    """(frames, H, W) of `dtype`: one scene, per-frame Gaussian noise of `sigma`, the odd rows cut at the planted offset b --
    frame[y][x] = scene[y][x + b] for odd y --, so the offset to find is p = -b.  The scene and the noise depend on the seed
    alone, not on b."""
    rs = np.random.RandomState(seed)
    img = scene(rs, H, W, blobs, P)
    noise = rs.normal(0.0, 1.0, size=(frames, H, W + 2 * P)) * sigma
    full = np.rint(img[None] + noise)
    out = full[:, :, P:P + W].copy()
    out[:, 1::2, :] = full[:, 1::2, P + b:P + b + W]
    return out.astype(dtype)


# (H, W, P, blobs, noise sigma, frames, seeds): the oracle recovers every planted offset in (-P, P) from the totals
CONFIGS = [(24, 40, 4, 12, 0, 1, 8), (24, 40, 4, 12, 0, 4, 8), (24, 40, 4, 12, 20, 1, 8), (24, 40, 4, 12, 20, 4, 8),
           (32, 64, 8, 20, 20, 4, 4), (33, 80, 16, 30, 20, 4, 3), (16, 24, 3, 6, 10, 2, 10)]
NOISY = (32, 64, 8, 20, 60, 8, 4)     # the totals still recover all; single frames do not
