"""Temporal binning restated for the tests (include/dcunet.h, dc_series_bin_time): the rounded means of b consecutive frames on
int64 sums, the same per pixel in Python integers, and the streaming form with (carry, phase) of the C contract.  numpy only;
shares no code with the product."""
import numpy as np

MAX_BIN_FRAMES = 64


def bin_time(frames, b):
    """(T,H,W) int16 / uint16 -> (T // b, H, W) of the same dtype: floor((2 s + b) / (2 b)) of the exact sum s of every b
    consecutive frames (numpy's // floors, for negative sums too); the trailing T % b frames are dropped."""
    frames = np.asarray(frames)
    T = frames.shape[0]
    n = T // b
    s = frames[:n * b].astype(np.int64).reshape((n, b) + frames.shape[1:]).sum(axis=1)
    return ((2 * s + b) // (2 * b)).astype(frames.dtype)


def bin_time_naive(frames, b):
    """The same, pixel by pixel in Python integers, by the words of the contract: the mean rounded half up."""
    frames = np.asarray(frames)
    T, H, W = frames.shape
    out = np.zeros((T // b, H, W), frames.dtype)
    for j in range(T // b):
        for y in range(H):
            for x in range(W):
                s = sum(int(frames[j * b + i, y, x]) for i in range(b))
                q, r = divmod(s, b)                      # s = q b + r, 0 <= r < b, for negative s too
                out[j, y, x] = q + (1 if 2 * r >= b else 0)
    return out


def stream(chunk, b, phase, carry):
    """One call of the C contract: chunk (tc,H,W), carry int64 (H,W) = the sum of the `phase` frames of the open bin (read only
    when phase > 0) -> (out (n_out,H,W), the new carry or None where the call leaves no bin open, the new phase)."""
    chunk = np.asarray(chunk)
    tc = chunk.shape[0]
    assert 0 <= phase < b
    out, s, k = [], (np.array(carry, np.int64) if phase > 0 else np.zeros(chunk.shape[1:], np.int64)), phase
    for i in range(tc):
        s = s + chunk[i].astype(np.int64)
        k += 1
        if k == b:
            out.append(((2 * s + b) // (2 * b)).astype(chunk.dtype))
            s, k = np.zeros(chunk.shape[1:], np.int64), 0
    out = np.stack(out) if out else np.zeros((0,) + chunk.shape[1:], chunk.dtype)
    assert out.shape[0] == (phase + tc) // b and k == (phase + tc) % b
    return out, (s if k > 0 else None), k


def stream_all(frames, b, cuts):
    """frames cut at the indices `cuts` and passed through stream() chunk by chunk -> the concatenated output."""
    frames = np.asarray(frames)
    edges = [0] + list(cuts) + [frames.shape[0]]
    carry, phase, outs = None, 0, []
    for lo, hi in zip(edges[:-1], edges[1:]):
        if hi > lo:
            out, new, phase = stream(frames[lo:hi], b, phase, carry)
            carry = new if new is not None else carry        # a call that closes its last bin leaves carry as it was
            outs.append(out)
    return np.concatenate(outs) if outs else np.zeros((0,) + frames.shape[1:], frames.dtype)
