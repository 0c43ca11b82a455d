"""Times of the temporal binning on one GPU (the figures of DESIGN.md section 4b, "Temporal binning: times").

    python scripts/temporal_bin_speed.py [--hw 512] [--chunk 64] [--out FILE]

One chunk of `--chunk` int16 frames of `--hw` x `--hw`, random over the whole range.  Timed per chunk: dc_series_bin_time at b = 2,
4, 8 and 16 from an empty carry, and at b = 4 from a carried head (phase 1: the items of slot 0 read carry and write the open bin's)
-- beside the H2D copy of the chunk out of pinned memory and dc_bidi_apply on the same chunk, which moves the chunk's bytes in and
the same out where the binning writes 1 / b of them.  HIP events on the launch stream around 5 launches back to back; every row is
warmed up once, then ONE run takes 5 rounds in which all rows are timed one after the other (the variants interleaved, so that a
drift of the clock meets all of them alike); the figure is the median of a row's 5 samples (min - max).  Every variant's output is
compared with numpy before it is timed.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BINS = (2, 4, 8, 16)


def rounded_means(frames, b):
    n = frames.shape[0] // b
    s = frames[:n * b].astype(np.int64).reshape((n, b) + frames.shape[1:]).sum(axis=1)
    return ((2 * s + b) // (2 * b)).astype(frames.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hw', type=int, default=512)
    ap.add_argument('--chunk', type=int, default=64)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from deep_calcium_amd._lib import lib
    L = lib()
    H = W = args.hw
    C = args.chunk
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    nbytes = C * H * W * 2
    say('temporal binning, one chunk of %d x %d x %d int16 (%.1f MB), %s' % (C, H, W, nbytes / 1e6, torch.cuda.get_device_name(0)))
    stream = torch.cuda.current_stream().cuda_stream
    rs = np.random.RandomState(0)
    raw = rs.randint(-32768, 32768, size=(C, H, W)).astype(np.int16)

    def timed(fn, reps=5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    host = torch.from_numpy(raw.copy()).pin_memory()
    dev = torch.empty((C, H, W), dtype=torch.int16, device='cuda')
    dev.copy_(host)
    out = torch.empty((C, H, W), dtype=torch.int16, device='cuda')
    carry = torch.zeros((H * W,), dtype=torch.int32, device='cuda')

    def bin_time(b, phase):
        return lambda: L.dc_series_bin_time(dev.data_ptr(), 0, C, H, W, b, phase, carry.data_ptr(), out.data_ptr(), stream)

    for b in BINS:                                       # what is timed is right
        bin_time(b, 0)()
        assert np.array_equal(out[:C // b].cpu().numpy(), rounded_means(raw, b)), b
    rows = [('h2d', 'H2D copy of the chunk (pinned)', nbytes, lambda: dev.copy_(host, non_blocking=True)),
            ('apply', 'dc_bidi_apply', 2 * nbytes, lambda: L.dc_bidi_apply(dev.data_ptr(), C, 3, H, W, 0, out.data_ptr(), stream))]
    for b in BINS:
        rows.append((('bin', b), 'dc_series_bin_time, b = %d' % b, nbytes + nbytes // b, bin_time(b, 0)))
    rows.append(('carried', 'dc_series_bin_time, b = 4, phase 1', nbytes + (C + 1) // 4 * H * W * 2 + 8 * H * W, bin_time(4, 1)))
    for _, _, _, fn in rows:                             # warm-up
        timed(fn, 1)
    samples = dict((key, []) for key, _, _, _ in rows)
    for _ in range(5):                                   # one run, the variants interleaved
        for key, _, _, fn in rows:
            samples[key].append(timed(fn))
    med = dict((k, (float(np.median(v)), min(v), max(v))) for k, v in samples.items())
    h2d = med['h2d'][0]
    say('per chunk, 5 launches back to back per sample, median of 5 interleaved samples after a warm-up (min - max), the bytes moved')
    say('per second (in + out), and the ratio to the copy:')
    for key, label, moved, _ in rows:
        ms, lo, hi = med[key]
        say('  %-36s %8.3f ms  (%.3f - %.3f)  %7.1f GB/s  / H2D = %5.2f' % (label, ms, lo, hi, moved / ms / 1e6, ms / h2d))
    worst = max(med[('bin', b)][0] for b in BINS)
    say('the slowest binning, %.3f ms, %s under the copy of %.3f ms; dc_bidi_apply takes %.3f ms'
        % (worst, 'stays' if worst < h2d else 'does NOT stay', h2d, med['apply'][0]))
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
