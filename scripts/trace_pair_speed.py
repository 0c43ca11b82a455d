"""Times of the ROI trace-pair correlation on one GPU (the figures of DESIGN.md section 4k, "Merging fragmented ROIs: times").

    python scripts/trace_pair_speed.py [--rois 300] [--frames 8192] [--hw 512] [--chunk 64] [--detrend 128] [--out FILE]

`--rois` rectangular ROIs of 100 to 400 pixels laid out at random in a `--hw` x `--hw` frame, their int64 sums over `--frames`
frames resident on the device (random values of the size ROI sums have).  Two pair sets: the neighbour pairs of the layout
(roi_neighbours at distance 2: what the merge step computes) and ALL R (R - 1) / 2 pairs (the worst case); two settings: one
segment (detrend None) and `--detrend` frames per segment.  Timed: dc_trace_pair_moments and dc_trace_pair_corr for each -- beside
dc_roi_trace_moments over the same sums, and beside what ONE 64-frame chunk of the streaming pass costs (its H2D copy out of pinned
memory and dc_roi_trace_accumulate on it): the pass makes `--frames` / 64 of those.  HIP events on the launch stream around 5
launches back to back; every row is warmed up once, then ONE run takes 5 rounds in which all rows are timed one after the other
(the variants interleaved, so that a drift of the clock meets all of them alike); the figure is the median of a row's 5 samples
(min - max).  Before anything is timed the neighbour pairs' numerators are compared with Python integers on a sample of pairs.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_rois(n, H, W, rs):
    rois = []
    for _ in range(n):
        h = int(rs.randint(10, 21))
        w = int(rs.randint(10, 21))                      # 100 .. 400 pixels
        y0, x0 = int(rs.randint(0, H - h)), int(rs.randint(0, W - w))
        rois.append(np.array([[y, x] for y in range(y0, y0 + h) for x in range(x0, x0 + w)], np.int64))
    return rois


def exact(x, y, plan):
    x, y = [int(v) for v in x], [int(v) for v in y]
    return sum(m * (n * sum(a * b for a, b in zip(x[t:t + n], y[t:t + n])) - sum(x[t:t + n]) * sum(y[t:t + n])) for t, n, m in plan)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rois', type=int, default=300)
    ap.add_argument('--frames', type=int, default=8192)
    ap.add_argument('--hw', type=int, default=512)
    ap.add_argument('--chunk', type=int, default=64)
    ap.add_argument('--detrend', type=int, default=128)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from deep_calcium_amd import RoiTraceExtractor, TracePairCorr, detrend_plan, roi_neighbours
    from deep_calcium_amd._lib import lib
    L = lib()
    H = W = args.hw
    R, T, C, D = args.rois, args.frames, args.chunk, args.detrend
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    rs = np.random.RandomState(0)
    rois = make_rois(R, H, W, rs)
    areas = np.array([len(r) for r in rois], np.int64)
    near = roi_neighbours(rois, (H, W), max_dist=2)
    every = np.array([(i, j) for i in range(R) for j in range(i + 1, R)], np.int32)
    say('trace-pair correlation, %d ROIs of %d to %d pixels x %d frames (%.1f MB of int64 sums), %d neighbour pairs at distance 2, %d pairs in all, %s'
        % (R, areas.min(), areas.max(), T, R * T * 8 / 1e6, len(near), len(every), torch.cuda.get_device_name(0)))
    stream = torch.cuda.current_stream().cuda_stream
    # sums of the size ROI sums have: a baseline of 400 per pixel, activity and noise on top
    sums = (400 * areas[:, None] + rs.randint(-30, 200, size=(R, T)) * np.sqrt(areas)[:, None].astype(np.int64)).astype(np.int64)
    dsums = torch.from_numpy(sums).cuda()

    # what is timed is right: a sample of the neighbour pairs against Python integers, both settings
    for seg in (None, D):
        tp = TracePairCorr(dsums, areas, near[:8], detrend_frames=seg)
        plan = detrend_plan(T, seg) if seg else [(0, T, 1)]
        for (i, j), m in zip(near[:8].tolist(), tp.result('moments')):
            assert (m['Nxx'], m['Nxy'], m['Nyy']) == (exact(sums[i], sums[i], plan), exact(sums[i], sums[j], plan), exact(sums[j], sums[j], plan))

    def timed(fn, reps=5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    sets = dict(near=torch.from_numpy(near).cuda(), all=torch.from_numpy(every).cuda())
    num = torch.empty((len(every), 6), dtype=torch.int64, device='cuda')
    corr = torch.empty((len(every),), dtype=torch.float32, device='cuda')
    rmom = torch.empty((3 * R,), dtype=torch.int64, device='cuda')
    raw = rs.randint(-32768, 32768, size=(C, H, W)).astype(np.int16)
    host = torch.from_numpy(raw).pin_memory()
    dev = torch.empty((C, H, W), dtype=torch.int16, device='cuda')
    dev.copy_(host)
    ext = RoiTraceExtractor((H, W), T, np.int16, rois, chunk_frames=C)

    def moments(which, seg):
        p = sets[which]
        return lambda: L.dc_trace_pair_moments(dsums.data_ptr(), T, R, T, seg, p.data_ptr(), len(p), num.data_ptr(), stream)

    def finalize(which):
        return lambda: L.dc_trace_pair_corr(num.data_ptr(), len(sets[which]), corr.data_ptr(), stream)

    def accumulate():
        L.dc_roi_trace_accumulate(dev.data_ptr(), 0, C, 0, ext._row_off.data_ptr(), ext._row_pix.data_ptr(), ext._row_roi.data_ptr(), ext._rows,
                                  ext.n_rois, ext.sums.data_ptr(), T, H, W, stream)

    rows = [('h2d', 'H2D copy of one chunk of %d frames (pinned)' % C, lambda: dev.copy_(host, non_blocking=True)),
            ('acc', 'dc_roi_trace_accumulate on that chunk', accumulate),
            ('rmom', 'dc_roi_trace_moments (%d rows)' % R, lambda: L.dc_roi_trace_moments(dsums.data_ptr(), T, R, T, rmom.data_ptr(), stream)),
            ('near0', 'dc_trace_pair_moments, %d neighbour pairs, one segment' % len(near), moments('near', 0)),
            ('nearL', 'dc_trace_pair_moments, %d neighbour pairs, L = %d' % (len(near), D), moments('near', D)),
            ('nearc', 'dc_trace_pair_corr, %d neighbour pairs' % len(near), finalize('near')),
            ('all0', 'dc_trace_pair_moments, all %d pairs, one segment' % len(every), moments('all', 0)),
            ('allL', 'dc_trace_pair_moments, all %d pairs, L = %d' % (len(every), D), moments('all', D)),
            ('allc', 'dc_trace_pair_corr, all %d pairs' % len(every), finalize('all'))]
    for _, _, fn in rows:                                # warm-up
        timed(fn, 1)
    samples = dict((key, []) for key, _, _ in rows)
    for _ in range(5):                                   # one run, the variants interleaved
        for key, _, fn in rows:
            samples[key].append(timed(fn))
    med = dict((k, (float(np.median(v)), min(v), max(v))) for k, v in samples.items())
    say('per call, 5 launches back to back per sample, median of 5 interleaved samples after a warm-up (min - max):')
    for key, label, _ in rows:
        ms, lo, hi = med[key]
        say('  %-62s %8.3f ms  (%.3f - %.3f)' % (label, ms, lo, hi))
    chunks = (T + C - 1) // C
    one_pass = chunks * max(med['h2d'][0], med['acc'][0])
    say('one streaming pass over %d frames is %d chunks: at least %d x %.3f ms = %.1f ms (the copy and the kernel overlap)'
        % (T, chunks, chunks, max(med['h2d'][0], med['acc'][0]), one_pass))
    for which, label in (('near', 'the merge step (neighbour pairs)'), ('all', 'all pairs')):
        for key, what in ((which + '0', 'one segment'), (which + 'L', 'L = %d' % D)):
            step = med[key][0] + med[which + 'c'][0]
            say('%s, %s: %.3f ms = %.4f of the pass, which %s small against it' % (label, what, step, step / one_pass,
                                                                                 'is' if step < 0.05 * one_pass else 'is NOT'))
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
