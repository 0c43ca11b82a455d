"""Times of the trace dynamics on one GPU (the figures of DESIGN.md section 4o and of the README's "Estimating the decay").

    python scripts/trace_dynamics_speed.py [--frames 8192] [--rois 512,4096] [--out FILE]

The traces are those of the reach table (events at rate 0.03 a frame, decay 8 frames, amplitude 1, Gaussian noise of sigma 0.3) as
float32, lying on the device.  Timed per trace count: dc_trace_noise, dc_trace_ar1_estimate (lags 5, the noise included),
dc_ar1_tables, dc_trace_deconv_ar1_each (per-trace decays: pick_gamma's g_each, tables built before) beside dc_trace_deconv_ar1
(the pooled decay, one table) on the same traces with the same s_min = 3 sigma_hat -- HIP events on the launch stream; outputs and
workspaces allocated once --, and dc_trace_ar1_estimate_host and numpy's trace_noise on ONE core of the same box by the wall
clock.  Every row is warmed up once, then ONE run takes 5 rounds in which all rows are timed one after the other (the variants
interleaved, so that a drift of the clock meets all of them alike); the figure is the median of a row's 5 samples (min - max).
A call is timed alone, its input just touched by the call before it: 512 traces (16 MiB of float32) stay resident in the 256 MiB
last-level cache between calls, 4096 traces (128 MiB) mostly do, their 256 MiB of float64 outputs do not.  Before anything is timed
the device result is compared with the host entry point's in every bit.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.trace_deconv_speed import traces       # noqa: E402  (the reach generator, R traces at once)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8192)
    ap.add_argument('--rois', default='512,4096')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from deep_calcium_amd._lib import lib
    from deep_calcium_amd.deconv import ar1_table, trace_noise
    from deep_calcium_amd.dynamics import pick_gamma
    L = lib()
    T, lags = args.frames, 5
    counts = [int(v) for v in args.rois.split(',')]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('trace dynamics, traces of %d frames, lags %d, %s; host: one core' % (T, lags, torch.cuda.get_device_name(0)))
    stream = torch.cuda.current_stream().cuda_stream
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                  # noqa: E731
    y_all = traces(max(counts), T)
    rows, keep = [], []
    for R in counts:
        y_h = np.ascontiguousarray(y_all[:R])
        y = torch.from_numpy(y_h).cuda()
        sigma = torch.empty(R, dtype=torch.float64, device='cuda')
        sigma2 = torch.empty(R, dtype=torch.float64, device='cuda')
        xc = torch.empty((R, lags + 1), dtype=torch.float64, device='cuda')
        g_raw = torch.empty(R, dtype=torch.float64, device='cuda')
        sigma_h, xc_h, g_h = np.empty(R), np.empty((R, lags + 1)), np.empty(R)

        def noise(R=R, y=y, sigma2=sigma2):
            L.dc_trace_noise(y.data_ptr(), 0, T, R, T, sigma2.data_ptr(), stream)

        def estimate(R=R, y=y, sigma=sigma, xc=xc, g_raw=g_raw):
            L.dc_trace_ar1_estimate(y.data_ptr(), 0, T, R, T, lags, None, sigma.data_ptr(), xc.data_ptr(), g_raw.data_ptr(), stream)

        def estimate_host(R=R, y_h=y_h, sigma_h=sigma_h, xc_h=xc_h, g_h=g_h):
            L.dc_trace_ar1_estimate_host(ptr(y_h), 0, T, R, T, lags, None, ptr(sigma_h), ptr(xc_h), ptr(g_h))

        def noise_numpy(y_h=y_h):
            trace_noise(y_h)

        # what is timed is right: the device against the host entry point and numpy, every bit
        noise()
        estimate()
        estimate_host()
        torch.cuda.synchronize()
        assert sigma.cpu().numpy().tobytes() == sigma_h.tobytes() == sigma2.cpu().numpy().tobytes() == trace_noise(y_h).tobytes()
        assert xc.cpu().numpy().tobytes() == xc_h.tobytes() and g_raw.cpu().numpy().tobytes() == g_h.tobytes()
        g_each_h, status, g_pool = pick_gamma(g_h)
        say('R = %d: device == host in every bit; g_raw min / median / max = %.4f / %.4f / %.4f, pooled %.4f (true %.4f), median sigma_hat %.3f'
            % (R, g_h.min(), float(np.median(g_h)), g_h.max(), g_pool, float(np.exp(-1.0 / 8.0)), float(np.median(sigma_h))))

        g_each = torch.from_numpy(g_each_h).cuda()
        tables = torch.empty((R, T + 1), dtype=torch.float64, device='cuda')
        table = torch.from_numpy(ar1_table(g_pool, T)).cuda()
        smin, lam = torch.from_numpy(3.0 * sigma_h).cuda(), torch.zeros(R, dtype=torch.float64, device='cuda')
        ws = torch.empty(L.dc_trace_deconv_ws_bytes(R, T) // 8, dtype=torch.float64, device='cuda')
        c = torch.empty((R, T), dtype=torch.float64, device='cuda')
        s = torch.empty((R, T), dtype=torch.float64, device='cuda')
        n = torch.empty(R, dtype=torch.int32, device='cuda')

        def build_tables(R=R, g_each=g_each, tables=tables):
            L.dc_ar1_tables(g_each.data_ptr(), R, T, tables.data_ptr(), T + 1, stream)

        def each(R=R, y=y, g_each=g_each, tables=tables, lam=lam, smin=smin, ws=ws, c=c, s=s, n=n):
            L.dc_trace_deconv_ar1_each(y.data_ptr(), 0, T, R, T, g_each.data_ptr(), tables.data_ptr(), T + 1, lam.data_ptr(), smin.data_ptr(),
                                       ws.data_ptr(), c.data_ptr(), s.data_ptr(), n.data_ptr(), stream)

        def shared(R=R, y=y, table=table, lam=lam, smin=smin, ws=ws, c=c, s=s, n=n, g_pool=g_pool):
            L.dc_trace_deconv_ar1(y.data_ptr(), 0, T, R, T, g_pool, table.data_ptr(), lam.data_ptr(), smin.data_ptr(), ws.data_ptr(), c.data_ptr(),
                                  s.data_ptr(), n.data_ptr(), stream)

        build_tables()
        keep.append((y, sigma, sigma2, xc, g_raw, g_each, tables, table, smin, lam, ws, c, s, n))
        rows += [(('noise', R), 'dc_trace_noise, %d traces' % R, noise, True),
                 (('est', R), 'dc_trace_ar1_estimate (noise included), %d traces' % R, estimate, True),
                 (('tab', R), 'dc_ar1_tables, %d traces' % R, build_tables, True),
                 (('each', R), 'dc_trace_deconv_ar1_each, %d traces' % R, each, True),
                 (('shared', R), 'dc_trace_deconv_ar1, %d traces' % R, shared, True),
                 (('host', R), 'dc_trace_ar1_estimate_host, one core, %d traces' % R, estimate_host, False),
                 (('numpy', R), 'numpy trace_noise, one core, %d traces' % R, noise_numpy, False)]

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
        say('  %-62s %10.3f ms  (%.3f - %.3f)' % (label, ms, lo, hi))
    for R in counts:
        m = dict((k, med[(k, R)][0]) for k in ('noise', 'est', 'tab', 'each', 'shared', 'host', 'numpy'))
        say('R = %d: the estimate takes %.3f of the one-core host build and the noise %.3f of numpy; each / shared = %.2f, and with the tables '
            'built (each + tables) / shared = %.2f; estimate / shared deconvolution = %.2f'
            % (R, m['est'] / m['host'], m['noise'] / m['numpy'], m['each'] / m['shared'], (m['each'] + m['tab']) / m['shared'], m['est'] / m['shared']))
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
