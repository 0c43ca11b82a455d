"""The oracle of sub-pixel motion correction: an independent restatement of the definitions in include/dcunet.h (refinement of a
pick, split of a fine shift, bilinear interpolation, fine shift field, fine valid rectangle) in Python integers and numpy int64.
Fine shifts are integers in sixteenths of a pixel; a fine shift (sy, sx) means out[y, x] = frame interpolated at (y + sy / 16,
x + sx / 16).  Everything is exact."""
import numpy as np

import _motion_block_ref as bref

Q = 16


def refine_q(sm, s0, sp):
    """q of one axis from the picked score s0 and its neighbours at -1 and +1: Python ints, so no 128-bit type is needed."""
    sm, s0, sp = int(sm), int(s0), int(sp)
    N, D = sm - sp, sm - 2 * s0 + sp
    assert D >= 0 and abs(N) <= D, 's0 is not the minimum of its neighbourhood'
    if D == 0:
        return 0
    m = (Q * abs(N) + D - 1) // (2 * D)
    return m if N > 0 else -m


def refine_entry(table, py, px):
    """(qy, qx) of the entry (py, px) of one (2R+1, 2R+1) table; 0 on an axis where the entry lies on the border; (0, 0) and
    nothing read for an entry outside the table."""
    R = (table.shape[0] - 1) // 2
    if not (-R <= py <= R and -R <= px <= R):
        return 0, 0
    i, j = py + R, px + R
    qy = refine_q(table[i - 1, j], table[i, j], table[i + 1, j]) if -R < py < R else 0
    qx = refine_q(table[i, j - 1], table[i, j], table[i, j + 1]) if -R < px < R else 0
    return qy, qx


def refine(scores, shifts):
    """(t, 2) int32 fine shifts from the (t, 2S+1, 2S+1) score tables and the (t, 2) picks."""
    scores, shifts = np.asarray(scores), np.asarray(shifts)
    out = np.zeros((len(scores), 2), np.int32)
    for t in range(len(scores)):
        dy, dx = int(shifts[t, 0]), int(shifts[t, 1])
        qy, qx = refine_entry(scores[t], dy, dx)
        out[t] = (Q * dy + qy, Q * dx + qx)
    return out


def block_refine(bscores, rigid, block_shifts, S):
    """(t, By, Bx, 2) int32 fine block shifts: the residual block_shifts - clamp(rigid, S) refined in the block's own table."""
    bscores, block_shifts = np.asarray(bscores), np.asarray(block_shifts)
    r = bref.clamp_rigid(rigid, S)
    T, By, Bx = bscores.shape[:3]
    out = np.zeros((T, By, Bx, 2), np.int32)
    for t in range(T):
        for i in range(By):
            for j in range(Bx):
                by, bx = int(block_shifts[t, i, j, 0]), int(block_shifts[t, i, j, 1])
                qy, qx = refine_entry(bscores[t, i, j], by - int(r[t, 0]), bx - int(r[t, 1]))
                out[t, i, j] = (Q * by + qy, Q * bx + qx)
    return out


def split(s):
    """(i, f): i = floor(s / 16), f = s - 16 i in [0, 16); Python ints or numpy int64 arrays."""
    i = s // Q                     # floor division for either sign
    return i, s - Q * i


def sample(frame, SY, SX, fill):
    """One frame interpolated at the per-pixel fine shifts SY, SX (int64 arrays that broadcast to the frame's shape)."""
    H, W = frame.shape
    yy, xx = np.mgrid[0:H, 0:W]
    iy, fy = split(np.broadcast_to(np.asarray(SY, np.int64), (H, W)))
    ix, fx = split(np.broadcast_to(np.asarray(SX, np.int64), (H, W)))
    y0, x0 = yy + iy, xx + ix
    y1, x1 = y0 + (fy > 0), x0 + (fx > 0)              # the taps that are used: row 1 only when fy > 0, column 1 only when fx > 0
    ok = (y0 >= 0) & (y1 < H) & (x0 >= 0) & (x1 < W)
    cy0, cy1, cx0, cx1 = (np.clip(v, 0, n - 1) for v, n in ((y0, H), (y1, H), (x0, W), (x1, W)))
    f = frame.astype(np.int64)
    a00, a01, a10, a11 = f[cy0, cx0], f[cy0, cx1], f[cy1, cx0], f[cy1, cx1]
    val = ((Q - fy) * ((Q - fx) * a00 + fx * a01) + fy * ((Q - fx) * a10 + fx * a11) + 128) // 256
    out = np.full((H, W), np.array(fill).astype(frame.dtype), frame.dtype)
    out[ok] = val[ok].astype(frame.dtype)
    return out


def apply_sub(frames, fine, fill=0):
    """out[t] = frames[t] interpolated at the fine shift fine[t]; any integer fine shift."""
    frames = np.asarray(frames)
    return np.stack([sample(frames[t], int(fine[t][0]), int(fine[t][1]), fill) for t in range(len(frames))])


def fine_field(fbs, H, W):
    """(H, W, 2) int64: the shift field of include/dcunet.h computed from one frame's FINE block shifts (By, Bx, 2)."""
    return bref.field(np.asarray(fbs).tolist(), H, W)


def warp_sub(frames, fine_bshifts, fill=0):
    frames = np.asarray(frames)
    T, H, W = frames.shape
    out = []
    for t in range(T):
        f = fine_field(fine_bshifts[t], H, W)
        out.append(sample(frames[t], f[:, :, 0], f[:, :, 1], fill))
    return np.stack(out)


def valid_fine(fine, shape):
    """((y0, y1), (x0, x1)) with y0 = max(0, -floor(min sy / 16)), y1 = H - max(0, ceil(max sy / 16)), likewise x."""
    H, W = shape
    s = [[int(v) for v in row] for row in np.asarray(fine).reshape(-1, 2)]
    lo = [min(r[c] for r in s) for c in (0, 1)]
    hi = [max(r[c] for r in s) for c in (0, 1)]
    return tuple((max(0, -(lo[c] // Q)), n - max(0, -((-hi[c]) // Q))) for c, n in ((0, H), (1, W)))
