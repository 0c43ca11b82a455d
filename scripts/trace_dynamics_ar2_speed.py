"""Times of the AR(2) estimate on one GPU (the figures of DESIGN.md section 4t and of the README's "Estimating the rise").

    python scripts/trace_dynamics_ar2_speed.py [--frames 8192] [--rois 512,4096] [--out FILE]

The traces are those of the AR(2) reach table (events at rate 0.03 a frame through the response of the roots exp(-1/8) and
exp(-1/2), peak 1, Gaussian noise of sigma 0.3) as float32, lying on the device.  Timed per trace count: dc_trace_ar2_solve at
lags 10 (the per-trace epilogue, on the xc and sigma the estimate wrote), dc_trace_ar1_estimate at lags 10 and at lags 5 in the
same run -- the O(R T) work is the estimate's, so what the feature costs is the difference between the two --, both by HIP events
on the launch stream with outputs allocated once, and dc_trace_ar2_solve_host on ONE core of the same box by the wall clock.
Every row is warmed up once, then ONE run takes 5 rounds in which all rows are timed one after the other (the variants
interleaved, so that a drift of the clock meets all of them alike); the figure is the median of a row's 5 samples (min - max).
A call is timed alone: a solve of a few microseconds is then mostly the launch itself.  Before anything is timed the device
result is compared with the host entry point's in every bit.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.trace_deconv_ar2_speed import traces       # noqa: E402  (the AR(2) reach generator, R traces at once)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8192)
    ap.add_argument('--rois', default='512,4096')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from deep_calcium_amd._lib import lib
    from deep_calcium_amd.dynamics import pick_roots
    L = lib()
    T = args.frames
    counts = [int(v) for v in args.rois.split(',')]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('AR(2) trace dynamics, traces of %d frames, %s; host: one core' % (T, torch.cuda.get_device_name(0)))
    stream = torch.cuda.current_stream().cuda_stream
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                  # noqa: E731
    y_all = traces(max(counts), T)
    rows, keep = [], []
    for R in counts:
        y = torch.from_numpy(np.ascontiguousarray(y_all[:R])).cuda()
        out = {}
        for lags in (10, 5):
            out[lags] = (torch.empty(R, dtype=torch.float64, device='cuda'), torch.empty((R, lags + 1), dtype=torch.float64, device='cuda'),
                         torch.empty(R, dtype=torch.float64, device='cuda'))
        g12 = torch.empty((R, 2), dtype=torch.float64, device='cuda')

        def estimate(lags, R=R, y=y, out=out):
            sigma, xc, g_raw = out[lags]
            L.dc_trace_ar1_estimate(y.data_ptr(), 0, T, R, T, lags, None, sigma.data_ptr(), xc.data_ptr(), g_raw.data_ptr(), stream)

        def solve(R=R, out=out, g12=g12):
            sigma, xc, _ = out[10]
            L.dc_trace_ar2_solve(xc.data_ptr(), R, T, 10, sigma.data_ptr(), g12.data_ptr(), stream)

        estimate(10)
        estimate(5)
        solve()
        torch.cuda.synchronize()
        xc_h, sigma_h, g12_h = out[10][1].cpu().numpy(), out[10][0].cpu().numpy(), np.empty((R, 2))

        def solve_host(R=R, xc_h=xc_h, sigma_h=sigma_h, g12_h=g12_h):
            L.dc_trace_ar2_solve_host(ptr(xc_h), R, T, 10, ptr(sigma_h), ptr(g12_h))

        solve_host()                                     # what is timed is right: the device against the host entry point, every bit
        assert g12.cpu().numpy().tobytes() == g12_h.tobytes()
        _, status, (d, r) = pick_roots(g12_h)
        say('R = %d: device == host in every bit; pooled d = %.4f (true %.4f), r = %.4f (true %.4f); status fine / complex / no rise / slow / '
            'undefined = %s' % (R, d, float(np.exp(-1.0 / 8.0)), r, float(np.exp(-1.0 / 2.0)), ' / '.join(str(v) for v in np.bincount(status, minlength=5))))
        keep.append((y, out, g12))
        rows += [(('solve', R), 'dc_trace_ar2_solve, lags 10, %d traces' % R, solve, True),
                 (('est10', R), 'dc_trace_ar1_estimate, lags 10 (noise included), %d traces' % R, lambda estimate=estimate: estimate(10), True),
                 (('est5', R), 'dc_trace_ar1_estimate, lags 5 (noise included), %d traces' % R, lambda estimate=estimate: estimate(5), True),
                 (('host', R), 'dc_trace_ar2_solve_host, one core, %d traces' % R, solve_host, False)]

    def timed(fn, on_gpu):
        if not on_gpu:
            t0 = time.perf_counter()
            fn()
            return (time.perf_counter() - t0) * 1e3
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    for _, _, fn, on_gpu in rows:                        # warm-up
        timed(fn, on_gpu)
    samples = dict((key, []) for key, _, _, _ in rows)
    for _ in range(5):                                   # one run, the variants interleaved
        for key, _, fn, on_gpu in rows:
            samples[key].append(timed(fn, on_gpu))
    med = dict((k, (float(np.median(v)), min(v), max(v))) for k, v in samples.items())
    say('per call, one call per sample, median of 5 interleaved samples after a warm-up (min - max):')
    for key, label, _, _ in rows:
        ms, lo, hi = med[key]
        say('  %-62s %10.4f ms  (%.4f - %.4f)' % (label, ms, lo, hi))
    for R in counts:
        m = dict((k, med[(k, R)][0]) for k in ('solve', 'est10', 'est5', 'host'))
        say('R = %d: five more lags cost %.4f ms (lags 10 / lags 5 = %.2f); the solve is %.4f of the estimate it follows and %.2f of its '
            'one-core host build' % (R, m['est10'] - m['est5'], m['est10'] / m['est5'], m['solve'] / m['est10'], m['solve'] / m['host']))
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
