"""Times of the series-summary path on one GPU (writes what profiles/series_summary.txt records).

    python scripts/series_summary_speed.py [--frames 3000] [--hw 512] [--out FILE]

A synthetic int16 recording is written as an .npz next to the output (np.savez: stored, so it is memory-mapped) and timed:
 (a) kernel time per chunk of dc_series_accumulate (with / without the float16 chain) and dc_series_accumulate_xy, HIP events
     on the launch stream, median of 5 after a warm-up, and the implied GB/s over the chunk's bytes;
 (b) the H2D copy of the same chunk out of pinned memory;
 (c) wall time of summarize_series_device for 'mean', 'mean16' and 'corr' (median of 5 after a warm-up, page cache warm);
 (d) the host paths on the same data: np.mean over the memmap, and the float16 loop of nf_datasets._populate as arithmetic only.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=3000)
    ap.add_argument('--hw', type=int, default=512)
    ap.add_argument('--out', default=None)
    ap.add_argument('--host-frames', type=int, default=None, help='frames of the float16 host loop (default: all)')
    args = ap.parse_args()
    import torch
    from deep_calcium_amd import series, summarize_series_device
    from deep_calcium_amd._lib import lib
    L = lib()
    T, H, W = args.frames, args.hw, args.hw
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('series summaries, %d x %d x %d int16 (%.2f GB), %s' % (T, H, W, T * H * W * 2 / 1e9, torch.cuda.get_device_name(0)))
    rs = np.random.RandomState(0)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, 'rec.npz')
    base = rs.randint(100, 1200, size=(1, H, W))
    raw = np.empty((T, H, W), np.int16)
    for t0 in range(0, T, 100):
        n = min(100, T - t0)
        raw[t0:t0 + n] = base + rs.randint(-90, 600, size=(n, H, W))
    np.savez(path, series_raw=raw, name=np.array('synthetic'))

    C = max(1, series._CHUNK_BYTES // (2 * H * W))
    chunk_bytes = C * H * W * 2
    say('chunk: %d frames = %.1f MB (the default of SeriesSummarizer)' % (C, chunk_bytes / 1e6))
    host = torch.from_numpy(raw[:C].copy()).pin_memory()
    dev = torch.empty((C, H, W), dtype=torch.int16, device='cuda')
    n = H * W
    st8 = [torch.zeros(n, dtype=torch.int64, device='cuda') for _ in range(2)]
    vmax = torch.zeros(n, dtype=torch.int32, device='cuda')
    m16, x16 = (torch.zeros(n, dtype=torch.int16, device='cuda') for _ in range(2))
    xy = torch.zeros((4, n), dtype=torch.int64, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    dev.copy_(host)
    acc = lambda chain: L.dc_series_accumulate(dev.data_ptr(), 0, C, C, T, m16.data_ptr() if chain else None,
                                               x16.data_ptr() if chain else None, st8[0].data_ptr(), st8[1].data_ptr(),
                                               vmax.data_ptr(), H, W, stream)
    rows = [('H2D copy of the chunk (pinned)', lambda: dev.copy_(host, non_blocking=True)),
            ('dc_series_accumulate (sums + float16 chain)', lambda: acc(True)),
            ('dc_series_accumulate (sums only)', lambda: acc(False)),
            ('dc_series_accumulate_xy', lambda: L.dc_series_accumulate_xy(dev.data_ptr(), 0, C, C, xy.data_ptr(), H, W, stream))]
    say('(a), (b) per chunk, median of 5 after a warm-up:')
    ms = {}
    for name, fn in rows:
        ms[name] = median_of(lambda: timed(fn))
        say('  %-46s %8.3f ms  %8.1f GB/s' % (name, ms[name], chunk_bytes / ms[name] / 1e6))
    h2d = ms[rows[0][0]]
    for name, _ in rows[1:]:
        say('  %s / H2D = %.2f  (%s)' % (name, ms[name] / h2d, 'below the copy' if ms[name] < h2d else 'ABOVE the copy'))

    say('(c) summarize_series_device, wall, median of 5 after a warm-up:')
    for kind in ('mean', 'mean16', 'corr'):
        def run():
            t = time.perf_counter()
            summarize_series_device(path, kind=kind)
            return time.perf_counter() - t
        s = median_of(run)
        say('  %-8s %8.3f s  (%.2f GB/s of recording)' % (kind, s, T * H * W * 2 / s / 1e9))

    say('(d) host paths on the same data:')
    frames, close = series._open_series(path, 'series/raw')
    def host_mean():
        t = time.perf_counter()
        np.mean(frames, axis=0)
        return time.perf_counter() - t
    say('  np.mean over the memmap              %8.3f s' % median_of(host_mean, n=3))
    nh = args.host_frames or T
    def host_loop():
        t = time.perf_counter()
        mean = np.zeros((H, W), np.float16)
        mx = np.zeros((H, W), np.int16)
        for img in frames[:nh]:
            mean = (mean + (img * 1. / T)).astype(np.float16)
            mx = np.maximum(mx, img)
        return (time.perf_counter() - t) * T / nh
    say('  float16 mean / int16 max loop (arithmetic only%s) %8.3f s' % (', scaled from %d frames' % nh if nh != T else '', median_of(host_loop, n=3, warm=0)))
    frames = None
    close()
    os.remove(path)
    os.rmdir(tmp)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
