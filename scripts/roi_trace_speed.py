"""Times of the ROI-trace path on one GPU (the figures of DESIGN.md section 4c).

    python scripts/roi_trace_speed.py [--frames 3000] [--hw 512] [--rois 300] [--out FILE]

A synthetic int16 recording is written as an .npz next to the output (np.savez: stored, so it is memory-mapped); the ROIs are
`--rois` discs of 100-400 pixels at random centres plus one whole-image ROI.  Timed:
 (a) kernel time per chunk of dc_roi_trace_accumulate (the ROIs cut into segments as rois_to_csr does, and uncut for comparison),
     HIP events on the launch stream around 20 launches back to back, median of 5 such samples after a warm-up, and the implied
     GB/s over the chunk's bytes;
 (b) the H2D copy of the same chunk out of pinned memory;
 (c) wall time of extract_traces_device for 'sum', 'mean' and 'zscore' (median of 5 after a warm-up, page cache warm), and of
     RoiTraceExtractor.feed on the recording already resident on the device;
 (d) the host equivalent on the same memmap: per ROI frames[:, ys, xs].sum(1).
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_of(fn, n=5, warm=1):
    for _ in range(warm):
        fn()
    return float(np.median([fn() for _ in range(n)]))


def make_rois(H, W, count, rs):
    """`count` discs of 100-400 pixels (clipped by the image border) + the whole image, as (k,2) [y,x] arrays."""
    yy, xx = np.mgrid[:H, :W]
    rois = []
    for _ in range(count):
        area = rs.randint(100, 401)
        rad2 = area / np.pi
        cy, cx = rs.randint(12, H - 12), rs.randint(12, W - 12)
        rois.append(np.argwhere((yy - cy) ** 2 + (xx - cx) ** 2 <= rad2))
    rois.append(np.argwhere(np.ones((H, W), bool)))
    return rois


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=3000)
    ap.add_argument('--hw', type=int, default=512)
    ap.add_argument('--rois', type=int, default=300)
    ap.add_argument('--out', default=None)
    ap.add_argument('--host-rois', type=int, default=None, help='ROIs of the host loop (default: all; the time is scaled by pixels)')
    args = ap.parse_args()
    import torch
    from deep_calcium_amd import RoiTraceExtractor, extract_traces_device, rois_to_csr, series
    from deep_calcium_amd._lib import lib
    L = lib()
    T, H, W = args.frames, args.hw, args.hw
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('ROI traces, %d x %d x %d int16 (%.2f GB), %s' % (T, H, W, T * H * W * 2 / 1e9, torch.cuda.get_device_name(0)))
    rs = np.random.RandomState(0)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, 'rec.npz')
    base = rs.randint(100, 1200, size=(1, H, W))
    raw = np.empty((T, H, W), np.int16)
    for t0 in range(0, T, 100):
        n = min(100, T - t0)
        raw[t0:t0 + n] = base + rs.randint(-90, 600, size=(n, H, W))
    np.savez(path, series_raw=raw, name=np.array('synthetic'))
    rois = make_rois(H, W, args.rois, rs)
    areas, row_off, row_pix, row_roi = rois_to_csr(rois, (H, W))
    R, S = len(areas), len(row_roi)
    say('%d ROIs, %d pixels listed (median area %d, largest %d), %d CSR rows of at most %d pixels'
        % (R, int(areas.sum()), int(np.median(areas)), int(areas.max()), S, int(np.diff(row_off).max())))

    C = max(1, series._CHUNK_BYTES // (2 * H * W))
    chunk_bytes = C * H * W * 2
    say('chunk: %d frames = %.1f MB (the default of RoiTraceExtractor)' % (C, chunk_bytes / 1e6))
    host = torch.from_numpy(raw[:C].copy()).pin_memory()
    dev = torch.empty((C, H, W), dtype=torch.int16, device='cuda')
    d_off, d_pix, d_roi = (torch.from_numpy(a).cuda() for a in (row_off, row_pix, row_roi))
    whole_off = torch.from_numpy(np.concatenate([[0], np.cumsum(areas)]).astype(np.int32)).cuda()
    sums = torch.zeros((R, 2 * C), dtype=torch.int64, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn, reps=1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    def clock():
        try:
            return '%d MHz' % torch.cuda.clock_rate()
        except Exception as e:                     # no SMI binding in this build
            return 'not read (%s)' % type(e).__name__

    dev.copy_(host)
    rows = [('H2D copy of the chunk (pinned)', lambda: dev.copy_(host, non_blocking=True)),
            ('dc_roi_trace_accumulate (segmented rows)',
             lambda: L.dc_roi_trace_accumulate(dev.data_ptr(), 0, C, C, d_off.data_ptr(), d_pix.data_ptr(), d_roi.data_ptr(), S, R,
                                               sums.data_ptr(), 2 * C, H, W, stream)),
            ('dc_roi_trace_accumulate (one row per ROI)',
             lambda: L.dc_roi_trace_accumulate(dev.data_ptr(), 0, C, C, whole_off.data_ptr(), d_pix.data_ptr(), None, R, R,
                                               sums.data_ptr(), 2 * C, H, W, stream))]
    say('(a), (b) per chunk, 20 back to back per sample, median of 5 samples after a warm-up (min - max); shader clock before: %s' % clock())
    ms = {}
    for name, fn in rows:
        timed(fn, 20)
        samples = [timed(fn, 20) for _ in range(5)]
        ms[name] = float(np.median(samples))
        say('  %-46s %8.3f ms  (%.3f - %.3f)  %8.1f GB/s' % (name, ms[name], min(samples), max(samples), chunk_bytes / ms[name] / 1e6))
    say('  shader clock after: %s' % clock())
    h2d = ms[rows[0][0]]
    for name, _ in rows[1:]:
        say('  %s / H2D = %.2f  (%s)' % (name, ms[name] / h2d, 'below the copy' if ms[name] < h2d else 'ABOVE the copy'))

    say('(c) extract_traces_device, wall, median of 5 after a warm-up:')
    for kind in ('sum', 'mean', 'zscore'):
        def run():
            t = time.perf_counter()
            extract_traces_device(path, rois, kind=kind)
            return time.perf_counter() - t
        s = median_of(run)
        say('  %-8s %8.3f s  (%.2f GB/s of recording)' % (kind, s, T * H * W * 2 / s / 1e9))

    def prep():
        t = time.perf_counter()
        rois_to_csr(rois, (H, W))
        return time.perf_counter() - t
    say('  of which rois_to_csr on the host        %8.3f s' % median_of(prep, n=3))
    resident = min(T, max(C, (2 << 30) // (2 * H * W)))
    dall = torch.from_numpy(raw[:resident]).cuda()
    ext = RoiTraceExtractor((H, W), resident, np.int16, rois)

    def fed():
        ext.fed = 0
        return timed(lambda: ext.feed(dall)) / 1e3
    s = median_of(fed)
    say('  RoiTraceExtractor.feed of %d resident frames  %8.4f s  (%.1f GB/s of recording)' % (resident, s, resident * H * W * 2 / s / 1e9))
    del dall, ext

    say('(d) the host equivalent, per ROI frames[:, ys, xs].sum(1) over the memmap:')
    frames, close = series._open_series(path, 'series/raw')
    nh = min(args.host_rois or len(rois), len(rois))
    pick = rois[len(rois) - nh:]                       # the whole-image ROI is the last one

    def host_loop():
        t = time.perf_counter()
        for c in pick:
            frames[:, c[:, 0], c[:, 1]].sum(1, dtype=np.int64)
        return (time.perf_counter() - t) * float(areas.sum()) / sum(len(c) for c in pick)
    say('  %d ROIs%s %8.3f s' % (nh, ' (scaled to all by pixels)' if nh != len(rois) else '', median_of(host_loop, n=3, warm=0)))
    frames = None
    close()
    os.remove(path)
    os.rmdir(tmp)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
