"""Times of the weighted ROI sums on one GPU (the figures of DESIGN.md section 4m, "Weighted traces: times").

    python scripts/weighted_trace_speed.py [--hw 512] [--chunk 64] [--rois 300] [--out FILE]

One chunk of `--chunk` frames of `--hw` x `--hw` int16, resident on the device, and `--rois` ROIs of 100 - 400 pixels each (discs
at random centres, so they overlap here and there; no ROI reaches the 512 pixels at which the extractor cuts rows, so every ROI is
one CSR row with its row_roi, the form the extractor launches).  Timed: dc_roi_wtrace_accumulate with weights in [1, 256] beside
dc_roi_trace_accumulate on the same rows and the chunk's H2D copy out of pinned memory.  HIP events on the launch stream around 20
launches back to back; every row is warmed up once, then ONE run takes 5 rounds in which all rows are timed one after the other (the
variants interleaved, so that a drift of the clock meets all of them alike); the figure is the median of a row's 5 samples (min -
max).  The chunk stays in the last-level cache between launches: these are not HBM rates.  Before anything is timed the sums of three
ROIs in three frames are compared with Python integers.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hw', type=int, default=512)
    ap.add_argument('--chunk', type=int, default=64)
    ap.add_argument('--rois', type=int, default=300)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from deep_calcium_amd._lib import lib
    L = lib()
    H = W = args.hw
    C, R = args.chunk, args.rois
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    stream = torch.cuda.current_stream().cuda_stream
    rs = np.random.RandomState(0)
    raw = (400 + 30 * rs.standard_normal((C, H, W))).astype(np.int16)
    yy, xx = np.mgrid[-12:13, -12:13]
    pix, wgt = [], []
    for r in range(R):
        area = rs.randint(100, 401)
        cy, cx = rs.randint(12, H - 12), rs.randint(12, W - 12)
        near = np.argsort((yy * yy + xx * xx).reshape(-1), kind='stable')[:area]          # the `area` pixels nearest the centre
        flat = np.sort((yy.reshape(-1)[near] + cy) * W + xx.reshape(-1)[near] + cx)
        pix.append(flat)
        wgt.append(rs.randint(1, 257, area))
    off = np.concatenate([[0], np.cumsum([len(p) for p in pix])])
    say('weighted ROI sums, one chunk of %d frames of %d x %d int16 (%.1f MB), %d ROIs of %d - %d pixels (%d entries), %s'
        % (C, H, W, C * H * W * 2 / 1e6, R, min(len(p) for p in pix), max(len(p) for p in pix), off[-1], torch.cuda.get_device_name(0)))
    host = torch.from_numpy(raw).pin_memory()
    dev = torch.empty((C, H, W), dtype=torch.int16, device='cuda')
    dev.copy_(host)
    d_off = torch.from_numpy(off.astype(np.int32)).cuda()
    d_pix = torch.from_numpy(np.concatenate(pix).astype(np.int32)).cuda()
    d_wgt = torch.from_numpy(np.concatenate(wgt).astype(np.uint16).view(np.int16)).cuda()
    d_roi = torch.arange(R, dtype=torch.int32, device='cuda')
    sums = torch.empty((R, C), dtype=torch.int64, device='cuda')
    wsums = torch.empty((R, C), dtype=torch.int64, device='cuda')

    def plain():
        L.dc_roi_trace_accumulate(dev.data_ptr(), 0, C, 0, d_off.data_ptr(), d_pix.data_ptr(), d_roi.data_ptr(), R, R, sums.data_ptr(), C, H, W,
                                  stream)

    def weighted():
        L.dc_roi_wtrace_accumulate(dev.data_ptr(), 0, C, 0, d_off.data_ptr(), d_pix.data_ptr(), d_wgt.data_ptr(), d_roi.data_ptr(), R, R,
                                   wsums.data_ptr(), C, H, W, stream)

    # what is timed is right: three ROIs in three frames against Python integers
    plain()
    weighted()
    got, gotw = sums.cpu().numpy(), wsums.cpu().numpy()
    flat = raw.reshape(C, -1)
    for r in (0, R // 2, R - 1):
        for f in (0, C // 2, C - 1):
            x = [int(flat[f, p]) for p in pix[r]]
            assert got[r, f] == sum(x) and gotw[r, f] == sum(int(w) * v for w, v in zip(wgt[r], x)), (r, f)

    def timed(fn, reps=20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    rows = [('h2d', 'H2D copy of the chunk (pinned)', lambda: dev.copy_(host, non_blocking=True)),
            ('plain', 'dc_roi_trace_accumulate', plain),
            ('wgt', 'dc_roi_wtrace_accumulate', weighted)]
    for _, _, fn in rows:                                # warm-up
        timed(fn, 1)
    samples = dict((key, []) for key, _, _ in rows)
    for _ in range(5):                                   # one run, the variants interleaved
        for key, _, fn in rows:
            samples[key].append(timed(fn))
    med = dict((k, (float(np.median(v)), min(v), max(v))) for k, v in samples.items())
    say('per call, 20 launches back to back per sample, median of 5 interleaved samples after a warm-up (min - max):')
    for key, label, _ in rows:
        ms, lo, hi = med[key]
        say('  %-40s %8.3f ms  (%.3f - %.3f)' % (label, ms, lo, hi))
    say('weighted / unweighted: %.2f; weighted = %.3f of the H2D copy: it %s under the copy (cache-resident chunk: not an HBM rate)'
        % (med['wgt'][0] / med['plain'][0], med['wgt'][0] / med['h2d'][0], 'hides' if med['wgt'][0] < med['h2d'][0] else 'DOES NOT hide'))
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
