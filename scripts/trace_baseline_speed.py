"""Times of the dF/F path on one GPU (the figures of DESIGN.md section 4g).

    python scripts/trace_baseline_speed.py [--rois 512] [--frames 8192] [--window 1801] [--percentile 8] [--host-rois 8] [--out FILE]

Synthetic int64 ROI sums as dc_roi_trace_accumulate would leave them (ROIs of 100-400 pixels of a bleaching 16-bit recording
with noise and transients, rings of 600-1500 pixels), resident on the device.  Timed, HIP events on the launch stream, median of 5
after a warm-up:
 (a) dc_trace_baseline alone, on the plain numerators (N = S) and on the neuropil-corrected ones (N = 256 An S - a A Sn, whose
     value range -- and with it the number of bisection rounds -- is 256 An times larger);
 (b) dc_trace_combine and dc_trace_scale;
 (c) the same baseline on the host: numpy's sliding_window_view + np.partition over the interior windows of `--host-rois` rows,
     scaled to all rows (the clipped windows at both ends are left out, in the host's favour).
The bisection round count is printed too: per (ROI, tile of 256 frames) the kernel needs ceil(log2(max - min + 1)) rounds over
the staged span at most.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TILE = 256


def synthetic_sums(R, T, rs, area_lo, area_hi):
    """(areas, sums): per pixel a bleaching level of 300-900 counts, photon-like noise, and for ROIs sparse decaying transients."""
    areas = rs.randint(area_lo, area_hi + 1, size=R).astype(np.int64)
    t = np.arange(T)
    level = rs.randint(300, 901, size=(R, 1)) * (0.75 + 0.25 * np.exp(-t / (0.4 * T)))[None, :]
    events = (rs.rand(R, T) < 0.002) * rs.randint(100, 600, size=(R, T))
    kernel = np.exp(-np.arange(60) / 15.0)
    trans = np.stack([np.convolve(e, kernel)[:T] for e in events])
    noise = rs.randn(R, T) * np.sqrt(level / areas[:, None]) * 3
    return areas, np.rint((level + trans + noise) * areas[:, None]).astype(np.int64)


def rounds(num, half):
    """ceil(log2(max - min + 1)) over the span every (row, tile) stages: the most rounds a thread of that workgroup runs."""
    R, T = num.shape
    out = []
    for tile0 in range(0, T, TILE):
        span = num[:, max(0, tile0 - half):min(T, tile0 + TILE + half)]
        width = (span.max(1) - span.min(1)).astype(object)
        out.append([int(w).bit_length() for w in width])
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rois', type=int, default=512)
    ap.add_argument('--frames', type=int, default=8192)
    ap.add_argument('--window', type=int, default=1801)
    ap.add_argument('--percentile', type=int, default=8)
    ap.add_argument('--host-rois', type=int, default=8, help='rows of the host baseline (the time is scaled to all rows)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from deep_calcium_amd import dff
    from deep_calcium_amd._lib import lib
    L = lib()
    R, T, q = args.rois, args.frames, args.percentile
    half = dff.window_half(args.window)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('dF/F baseline, R = %d, T = %d, window = %d, q = %d, %s' % (R, T, args.window, q, torch.cuda.get_device_name(0)))
    rs = np.random.RandomState(0)
    A, S = synthetic_sums(R, T, rs, 100, 400)
    An, Sn = synthetic_sums(R, T, rs, 600, 1500)
    ca, cb, cc, den, _ = dff.combine_coefficients(A, An, 0.7, 0)
    plain = S
    corrected = ca[:, None] * S - cb[:, None] * Sn + cc[:, None]
    stream = torch.cuda.current_stream().cuda_stream
    d_sums = torch.from_numpy(np.concatenate([S, Sn])).cuda()
    d_row = torch.from_numpy((R + np.arange(R)).astype(np.int32)).cuda()
    d_ca, d_cb, d_cc, d_den = (torch.from_numpy(x).cuda() for x in (ca, cb, cc, den))
    d_num = torch.empty((R, T), dtype=torch.int64, device='cuda')
    d_base = torch.empty((R, T), dtype=torch.int64, device='cuda')
    d_dff = torch.empty((R, T), dtype=torch.float32, device='cuda')
    d_f = torch.empty((R, T), dtype=torch.float32, device='cuda')

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def median(fn, n=5):
        timed(fn)
        samples = [timed(fn) for _ in range(n)]
        return float(np.median(samples)), min(samples), max(samples)

    say('(a) dc_trace_baseline (base and dff), median of 5 after a warm-up (min - max):')
    gpu_ms = {}
    for name, num in (('plain numerators N = S', plain), ('neuropil-corrected numerators', corrected)):
        d_in = torch.from_numpy(num).cuda()
        ms, lo, hi = median(lambda: L.dc_trace_baseline(d_in.data_ptr(), T, R, T, half, q, d_base.data_ptr(), d_dff.data_ptr(), stream))
        rd = rounds(num, half)
        steps = float(R) * T * min(args.window, T) * float(np.mean(rd))
        gpu_ms[name] = ms
        say('  %-34s %9.3f ms  (%.3f - %.3f)   bisection rounds per tile: median %d, max %d;  ~%.2e compare-and-count steps, %.2e per s'
            % (name, ms, lo, hi, int(np.median(rd)), int(rd.max()), steps, steps / ms * 1e3))
        if name.startswith('plain'):
            got = d_base[:args.host_rois].cpu().numpy()
    say('(b) the element-wise kernels:')
    ms, lo, hi = median(lambda: L.dc_trace_combine(d_sums.data_ptr(), T, d_row.data_ptr(), d_ca.data_ptr(), d_cb.data_ptr(), d_cc.data_ptr(), R,
                                                  T, d_num.data_ptr(), stream))
    say('  %-34s %9.3f ms  (%.3f - %.3f)' % ('dc_trace_combine', ms, lo, hi))
    ms, lo, hi = median(lambda: L.dc_trace_scale(d_num.data_ptr(), T, d_den.data_ptr(), R, T, d_f.data_ptr(), stream))
    say('  %-34s %9.3f ms  (%.3f - %.3f)' % ('dc_trace_scale', ms, lo, hi))

    nh = max(1, min(args.host_rois, R))
    n = 2 * half + 1
    if T >= n:
        k = dff.rank_index(q, n)
        t0 = time.perf_counter()
        view = np.lib.stride_tricks.sliding_window_view(plain[:nh], n, axis=1)
        host = np.stack([np.partition(v, k, axis=1)[:, k] for v in view])
        sec = (time.perf_counter() - t0) * R / nh
        same = np.array_equal(host, got[:nh, half:T - half])
        say('(c) numpy on the host, sliding_window_view + np.partition, %d rows scaled to %d, interior windows only: %9.2f s  (%s the device)'
            % (nh, R, sec, 'equal to' if same else 'DIFFERENT FROM'))
        say('    host / dc_trace_baseline = %.0f (plain numerators)' % (sec * 1e3 / gpu_ms['plain numerators N = S']))
    else:
        say('(c) skipped: the trace is shorter than one window')
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
