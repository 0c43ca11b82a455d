"""Times of the frame quality kernels on one GPU (the figures of DESIGN.md section 4l, "Artefact frames: times").

    python scripts/frame_quality_speed.py [--hw 512] [--chunk 64] [--out FILE]

One chunk of `--chunk` frames of `--hw` x `--hw` int16, resident on the device.  Timed: dc_frame_moments without and with a
template (whole frame, and the rectangle a registration within +-8 pixels leaves, which starts at an odd column), dc_frame_quality
on the chunk's moments, dc_frame_gather of every other frame and of all but three -- beside the chunk's H2D copy out of pinned
memory and dc_bidi_scores(P = 8) on the same chunk, the other per-chunk score the pipeline computes.  HIP events on the launch stream
around 20 launches back to back; every row is warmed up once, then ONE run takes 5 rounds in which all rows are timed one after
the other (the variants interleaved, so that a drift of the clock meets all of them alike); the figure is the median of a row's 5
samples (min - max).  The chunk stays in the caches between launches: these are not HBM rates.  Before anything is timed the
moments of three frames are compared with Python integers.
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

    say('frame quality, one chunk of %d frames of %d x %d int16 (%.1f MB), %s' % (C, H, W, C * H * W * 2 / 1e6, torch.cuda.get_device_name(0)))
    stream = torch.cuda.current_stream().cuda_stream
    rs = np.random.RandomState(0)
    raw = (400 + 30 * rs.standard_normal((C, H, W))).astype(np.int16)
    tmpl_h = (400 + 30 * rs.standard_normal((H, W))).astype(np.int16)
    host = torch.from_numpy(raw).pin_memory()
    dev = torch.empty((C, H, W), dtype=torch.int16, device='cuda')
    dev.copy_(host)
    tmpl = torch.from_numpy(tmpl_h).cuda()
    mom = torch.empty((C, 3), dtype=torch.int64, device='cuda')
    mean = torch.empty((C,), dtype=torch.float32, device='cuda')
    corr = torch.empty((C,), dtype=torch.float32, device='cuda')
    out = torch.empty((C, H, W), dtype=torch.int16, device='cuda')
    scores = torch.empty((C, 17), dtype=torch.int64, device='cuda')
    other = torch.arange(0, C, 2, dtype=torch.int32, device='cuda')
    most = torch.tensor([t for t in range(C) if t not in (C // 5, C // 2, C - 2)], dtype=torch.int32, device='cuda')
    whole = (0, H, 0, W)
    inner = (8, H - 8, 7, W - 8)                         # an odd first column: the rows need the alignment prologue

    def moments(t, rect):
        return lambda: L.dc_frame_moments(dev.data_ptr(), 0, C, t.data_ptr() if t is not None else None, H, W, rect[0], rect[1], rect[2], rect[3],
                                          mom.data_ptr(), stream)

    # what is timed is right: three frames against Python integers, both rectangles
    for rect in (whole, inner):
        moments(tmpl, rect)()
        got = mom.cpu().numpy()
        t = [int(v) for v in tmpl_h[rect[0]:rect[1], rect[2]:rect[3]].reshape(-1)]
        for f in (0, C // 2, C - 1):
            x = [int(v) for v in raw[f, rect[0]:rect[1], rect[2]:rect[3]].reshape(-1)]
            assert got[f].tolist() == [sum(x), sum(v * v for v in x), sum(v * w for v, w in zip(x, t))], (rect, f)
    tm = torch.empty((1, 3), dtype=torch.int64, device='cuda')
    L.dc_frame_moments(tmpl.data_ptr(), 0, 1, None, H, W, 0, H, 0, W, tm.data_ptr(), stream)
    ta, tb = (int(v) for v in tm.cpu().numpy()[0, :2])
    moments(tmpl, whole)()

    def timed(fn, reps=20):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    def gather(idx):
        return lambda: L.dc_frame_gather(dev.data_ptr(), C, idx.data_ptr(), int(idx.shape[0]), H, W, out.data_ptr(), stream)

    rows = [('h2d', 'H2D copy of the chunk (pinned)', lambda: dev.copy_(host, non_blocking=True)),
            ('bidi', 'dc_bidi_scores(P = 8)', lambda: L.dc_bidi_scores(dev.data_ptr(), 0, C, H, W, 8, scores.data_ptr(), stream)),
            ('m0', 'dc_frame_moments, no template, whole frame', moments(None, whole)),
            ('mt', 'dc_frame_moments, template, whole frame', moments(tmpl, whole)),
            ('mr', 'dc_frame_moments, template, rows 8.., columns 7..', moments(tmpl, inner)),
            ('q', 'dc_frame_quality, mean and corr of %d frames' % C,
             lambda: L.dc_frame_quality(mom.data_ptr(), C, H * W, ta, tb, mean.data_ptr(), corr.data_ptr(), stream)),
            ('g2', 'dc_frame_gather, every other frame (%d)' % int(other.shape[0]), gather(other)),
            ('g3', 'dc_frame_gather, all but three (%d)' % int(most.shape[0]), gather(most))]
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
        say('  %-62s %8.3f ms  (%.3f - %.3f)' % (label, ms, lo, hi))
    score = med['mt'][0] + med['q'][0]
    say('the scores of a chunk (moments with a template + quality): %.3f ms = %.2f of its H2D copy: they %s under the copy'
        % (score, score / med['h2d'][0], 'hide' if score < med['h2d'][0] else 'DO NOT hide'))
    say('the gather of a chunk (all but three): %.3f ms = %.2f of its H2D copy' % (med['g3'][0], med['g3'][0] / med['h2d'][0]))
    say('chunk bytes / time (cache-resident, not an HBM rate): moments with a template %.0f GB/s, gather of all but three %.0f GB/s (read + write)'
        % (C * H * W * 2 / med['mt'][0] / 1e6, 2 * int(most.shape[0]) * H * W * 2 / med['g3'][0] / 1e6))
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
