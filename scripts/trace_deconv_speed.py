"""Times of the AR(1) deconvolution on one GPU (the figures of DESIGN.md section 4n and of the README's "Spikes by deconvolution").

    python scripts/trace_deconv_speed.py [--frames 8192] [--rois 512,4096] [--out FILE]

The traces are those of the reach table (events at rate 0.03 a frame, decay 8 frames, amplitude 1, Gaussian noise of sigma 0.3) as
a fluorescence N = rint(4000 (1 + y)) in int64; dc_trace_baseline (window 1801, percentile 8) turns them into the float32 dF/F that
lies on the device, and that is what is deconvolved, with g = exp(-1/8) and s_min = 3 sigma_hat per trace.  Timed per trace count:
dc_trace_baseline, dc_trace_deconv_ar1 (forward + fill; workspace and outputs allocated once), the D2H copy of calcium and spikes
into pinned memory -- HIP events on the launch stream --, and dc_trace_deconv_ar1_host on ONE core of the same box by the wall
clock.  Every row is warmed up once, then ONE run takes 5 rounds in which all rows are timed one after the other (the variants
interleaved, so that a drift of the clock meets all of them alike); the figure is the median of a row's 5 samples (min - max).
Before anything is timed the device result is compared with the host entry point's in every bit.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def traces(R, T, sigma=0.3, seed=0):
    """The reach generator, R traces at once: the calcium by its recursion instead of a convolution with T taps."""
    rs = np.random.RandomState(seed)
    sp = rs.poisson(0.03, (R, T)) > 0
    g = np.exp(-1.0 / 8.0)
    c = np.empty((R, T))
    acc = np.zeros(R)
    for t in range(T):
        acc = acc * g + sp[:, t]
        c[:, t] = acc
    return np.float32(c + sigma * rs.standard_normal((R, T)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8192)
    ap.add_argument('--rois', default='512,4096')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from deep_calcium_amd._lib import lib
    from deep_calcium_amd.deconv import ar1_table, trace_noise
    L = lib()
    T = args.frames
    counts = [int(v) for v in args.rois.split(',')]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('AR(1) deconvolution, traces of %d frames, %s; host: one core' % (T, torch.cuda.get_device_name(0)))
    stream = torch.cuda.current_stream().cuda_stream
    g = float(np.exp(-1.0 / 8.0))
    G_h = ar1_table(g, T)
    G = torch.from_numpy(G_h).cuda()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                  # noqa: E731
    y_all = traces(max(counts), T)
    rows, state = [], {}
    for R in counts:
        num = torch.from_numpy(np.rint(4000.0 * (1.0 + y_all[:R].astype(np.float64))).astype(np.int64)).cuda()
        dff = torch.empty((R, T), dtype=torch.float32, device='cuda')
        L.dc_trace_baseline(num.data_ptr(), T, R, T, 900, 8, None, dff.data_ptr(), stream)
        dff_h = dff.cpu().numpy()
        smin_h = 3.0 * trace_noise(dff_h)
        lam_h = np.zeros(R)
        smin, lam = torch.from_numpy(smin_h).cuda(), torch.from_numpy(lam_h).cuda()
        ws = torch.empty(L.dc_trace_deconv_ws_bytes(R, T) // 8, dtype=torch.float64, device='cuda')
        c = torch.empty((R, T), dtype=torch.float64, device='cuda')
        s = torch.empty((R, T), dtype=torch.float64, device='cuda')
        n = torch.empty(R, dtype=torch.int32, device='cuda')
        c_h, s_h, n_h = np.empty((R, T)), np.empty((R, T)), np.empty(R, np.int32)
        pin_c, pin_s = torch.empty((R, T), dtype=torch.float64).pin_memory(), torch.empty((R, T), dtype=torch.float64).pin_memory()

        def device(R=R, dff=dff, lam=lam, smin=smin, ws=ws, c=c, s=s, n=n):
            L.dc_trace_deconv_ar1(dff.data_ptr(), 0, T, R, T, g, G.data_ptr(), lam.data_ptr(), smin.data_ptr(), ws.data_ptr(), c.data_ptr(),
                                  s.data_ptr(), n.data_ptr(), stream)

        def host(R=R, dff_h=dff_h, lam_h=lam_h, smin_h=smin_h, c_h=c_h, s_h=s_h, n_h=n_h):
            L.dc_trace_deconv_ar1_host(ptr(dff_h), 0, T, R, T, ptr(G_h), ptr(lam_h), ptr(smin_h), ptr(c_h), ptr(s_h), ptr(n_h))

        def baseline(R=R, num=num, dff=dff):
            L.dc_trace_baseline(num.data_ptr(), T, R, T, 900, 8, None, dff.data_ptr(), stream)

        def d2h(c=c, s=s, pin_c=pin_c, pin_s=pin_s):
            pin_c.copy_(c, non_blocking=True)
            pin_s.copy_(s, non_blocking=True)

        # what is timed is right: the device against the host entry point, every bit
        device()
        host()
        torch.cuda.synchronize()
        assert c.cpu().numpy().tobytes() == c_h.tobytes() and s.cpu().numpy().tobytes() == s_h.tobytes() and np.array_equal(n.cpu().numpy(), n_h)
        events = (s_h > 0).sum(1)
        say('R = %d: device == host in every bit; pools per trace median %d (max %d), events per trace median %d, median sigma_hat %.3f'
            % (R, int(np.median(n_h)), int(n_h.max()), int(np.median(events)), float(np.median(smin_h)) / 3.0))
        state[R] = (num, dff, ws, c, s, n, pin_c, pin_s)
        rows += [(('base', R), 'dc_trace_baseline (window 1801, q 8), %d traces' % R, baseline, True),
                 (('dev', R), 'dc_trace_deconv_ar1, %d traces' % R, device, True),
                 (('d2h', R), 'D2H copy of calcium and spikes (pinned), %d traces' % R, d2h, True),
                 (('host', R), 'dc_trace_deconv_ar1_host, one core, %d traces' % R, host, False)]

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
        dev, host, base, d2h = (med[(k, R)][0] for k in ('dev', 'host', 'base', 'd2h'))
        say('R = %d: the device takes %.2f of the one-core host build (%s), %.2f of the baseline kernel it follows, and its results take %.2f '
            'of its time to copy back; %.1f M samples/s' % (R, dev / host, 'FASTER' if dev < host else 'SLOWER', dev / base, d2h / dev,
                                                         R * T / dev / 1e3))
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
