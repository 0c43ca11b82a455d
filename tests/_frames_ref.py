"""The frame quality scores restated for the tests (include/dcunet.h, "Frame quality"), naive on purpose: the per-frame moments
as sums of Python integers, mean by Python's correctly rounded int / int, corr by an independent 60-digit decimal evaluation of
the exact quotient, and the gather, hold_index and flag_frames rules in plain loops over lists.  Shares no code with the product."""
import decimal

import numpy as np

MAX_PIXELS = 2 ** 28
_CTX = decimal.Context(prec=60)


def rect_of(shape, rect):
    H, W = shape
    return ((0, H), (0, W)) if rect is None else rect


def moments(frames, tmpl=None, rect=None):
    """frames (T,H,W) int16 / uint16, tmpl (H,W) or None -> [(a, b, c)] per frame, Python ints: the sums of x, x^2 and x * tmpl
    over rows [y0, y1), columns [x0, x1); c = 0 without a template."""
    (y0, y1), (x0, x1) = rect_of(frames.shape[1:], rect)
    t = None if tmpl is None else [int(v) for row in tmpl[y0:y1, x0:x1].tolist() for v in row]
    out = []
    for f in frames:
        x = [int(v) for row in f[y0:y1, x0:x1].tolist() for v in row]
        out.append((sum(x), sum(v * v for v in x), 0 if t is None else sum(v * w for v, w in zip(x, t))))
    return out


def moments_np(frames, tmpl=None, rect=None):
    """The same numbers by int64 numpy sums, for the long scenes of the reach test (exact: 2^28 pixels of 16 bits fit int64;
    tests/test_frames_api.py checks it against moments())."""
    (y0, y1), (x0, x1) = rect_of(frames.shape[1:], rect)
    x = frames[:, y0:y1, x0:x1].astype(np.int64).reshape(frames.shape[0], -1)
    c = np.zeros(x.shape[0], np.int64) if tmpl is None else (x * tmpl[y0:y1, x0:x1].astype(np.int64).reshape(1, -1)).sum(1)
    return [(int(a), int(b), int(cc)) for a, b, cc in zip(x.sum(1), (x * x).sum(1), c)]


def n_pixels(shape, rect=None):
    (y0, y1), (x0, x1) = rect_of(shape, rect)
    return (y1 - y0) * (x1 - x0)


def mean(a, n):
    """(float)((double)a / (double)n): Python's int / int is the correctly rounded quotient, and so is the double division of two
    integers below 2^53."""
    return np.float32(a / n)


def numerators(n, a, b, c, ta, tb):
    return n * b - a * a, n * c - a * ta, n * tb - ta * ta


def corr(n, a, b, c, ta, tb):
    """Nxt / sqrt(Nxx Ntt) in 60-digit decimal arithmetic, rounded once; exactly 0 where the frame or the template is constant."""
    nxx, nxt, ntt = numerators(n, a, b, c, ta, tb)
    if nxx <= 0 or ntt <= 0:
        return np.float32(0)
    return np.float32(float(_CTX.divide(decimal.Decimal(nxt), _CTX.sqrt(decimal.Decimal(nxx * ntt)))))


def scores(frames, tmpl=None, rect=None, mom=moments):
    """-> (moments int64 (T,3), mean float32 (T,), corr float32 (T,) or None)."""
    m = mom(frames, tmpl, rect)
    n = n_pixels(frames.shape[1:], rect)
    means = np.array([mean(a, n) for a, _, _ in m], np.float32)
    corrs = None
    if tmpl is not None:
        (ta, tb, _), = mom(tmpl[None], None, rect)
        corrs = np.array([corr(n, a, b, c, ta, tb) for a, b, c in m], np.float32)
    return np.array(m, np.int64).reshape(len(m), 3), means, corrs


def gather(frames, idx):
    """out[i] = frames[idx[i]], an all-zero frame for an index outside [0, T)."""
    T = frames.shape[0]
    out = np.zeros((len(idx),) + frames.shape[1:], frames.dtype)
    for i, t in enumerate(idx):
        if 0 <= int(t) < T:
            out[i] = frames[int(t)]
    return out


def hold_index(keep):
    """For every frame the latest kept frame at or before it; the first kept frame for a leading run of dropped frames."""
    keep = [bool(v) for v in keep]
    first = keep.index(True)
    out, last = [], first
    for t, k in enumerate(keep):
        if k:
            last = t
        out.append(last)
    return out


def _median(v):
    s = sorted(v)
    n = len(s)
    return s[n // 2] if n % 2 else (s[n // 2 - 1] + s[n // 2]) / 2.0


def _scale(v):
    med = _median(v)
    return med, 1.4826 * _median([abs(x - med) for x in v])


def flag_frames(mean_v, corr_v=None, k=8.0):
    """-> keep as a list of bools, in Python floats (float64): |mean - med| > k s drops; so does med_c - corr > k s_c."""
    m = [float(x) for x in mean_v]
    med, s = _scale(m)
    keep = [not abs(x - med) > k * s for x in m]
    if corr_v is not None:
        c = [float(x) for x in corr_v]
        med_c, s_c = _scale(c)
        keep = [kp and not med_c - x > k * s_c for kp, x in zip(keep, c)]
    return keep


def template_of(frames, n=200):
    """The mean of the first n frames rounded half up, in the frames' type: make_template without registration."""
    head = frames[:n].astype(np.int64)
    m = head.shape[0]
    return ((2 * head.sum(0) + m) // (2 * m)).astype(frames.dtype)


def plant(frames, seed, n=3, height=2000):
    """`n` flash frames, `height` grey levels up, chosen by RandomState(5000 + seed) -> (frames with them, their sorted indices)."""
    idx = np.sort(np.random.RandomState(5000 + seed).choice(frames.shape[0], n, replace=False))
    out = frames.copy()
    out[idx] = (out[idx].astype(np.int64) + height).astype(frames.dtype)
    return out, idx
