"""Times of the AR(2) deconvolution on one GPU (the figures of DESIGN.md section 4r and of the README's "A rise time in the
deconvolution (AR(2))").

    python scripts/trace_deconv_ar2_speed.py [--frames 8192] [--rois 512,4096] [--out FILE]

The traces are the reach generator's events (rate 0.03 a frame) convolved with the AR(2) kernel of the roots d = exp(-1/8) and
r = exp(-1/2) scaled to peak 1, with Gaussian noise of sigma 0.3, as float32 on the device.  Timed per trace count, with
s_min = 2 sigma_hat per trace for both models: dc_trace_deconv_ar2 (forward + fill; workspace and outputs allocated once) beside
dc_trace_deconv_ar1 of the same library at g = d on the same traces -- HIP events on the launch stream --, and
dc_trace_deconv_ar2_host on ONE core of the same box by the wall clock.  Every row is warmed up once, then ONE run takes 5 rounds in
which all rows are timed one after the other (the variants interleaved, so that a drift of the clock meets all of them alike); the
figure is the median of a row's 5 samples (min - max).  Before anything is timed the device result is compared with the host entry
point's in every bit.
"""
import argparse
import ctypes
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

D, RISE = math.exp(-1.0 / 8.0), math.exp(-1.0 / 2.0)


def traces(R, T, sigma=0.3, seed=0):
    """R traces at once: the calcium by its recursion instead of a convolution with T taps, scaled so that one event peaks at 1."""
    rs = np.random.RandomState(seed)
    sp = rs.poisson(0.03, (R, T)) > 0
    g1, g2 = D + RISE, -(D * RISE)
    k = np.arange(64)
    peak = ((D ** (k + 1) - RISE ** (k + 1)) / (D - RISE)).max()
    c = np.empty((R, T))
    c1, c2 = np.zeros(R), np.zeros(R)
    for t in range(T):
        c0 = g1 * c1 + g2 * c2 + sp[:, t]
        c[:, t] = c0
        c1, c2 = c0, c1
    return np.float32(c / peak + sigma * rs.standard_normal((R, T)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8192)
    ap.add_argument('--rois', default='512,4096')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from deep_calcium_amd._lib import lib
    from deep_calcium_amd.deconv import ar1_table, ar2_coefficients, ar2_table, trace_noise
    L = lib()
    T = args.frames
    counts = [int(v) for v in args.rois.split(',')]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('AR(2) deconvolution beside AR(1), traces of %d frames, %s; host: one core' % (T, torch.cuda.get_device_name(0)))
    stream = torch.cuda.current_stream().cuda_stream
    g1, g2 = ar2_coefficients(D, RISE)
    H_h, G_h = ar2_table(D, RISE, T), ar1_table(D, T)
    H, G = torch.from_numpy(H_h).cuda(), torch.from_numpy(G_h).cuda()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                  # noqa: E731
    y_all = traces(max(counts), T)
    rows = []
    for R in counts:
        y_h = np.ascontiguousarray(y_all[:R])
        y = torch.from_numpy(y_h).cuda()
        smin_h = 2.0 * trace_noise(y_h)
        lam_h = np.zeros(R)
        smin, lam = torch.from_numpy(smin_h).cuda(), torch.from_numpy(lam_h).cuda()
        ws2 = torch.empty(L.dc_trace_deconv_ar2_ws_bytes(R, T) // 8, dtype=torch.float64, device='cuda')
        ws1 = torch.empty(L.dc_trace_deconv_ws_bytes(R, T) // 8, dtype=torch.float64, device='cuda')
        c = torch.empty((R, T), dtype=torch.float64, device='cuda')
        s = torch.empty((R, T), dtype=torch.float64, device='cuda')
        n = torch.empty(R, dtype=torch.int32, device='cuda')
        c1 = torch.empty((R, T), dtype=torch.float64, device='cuda')
        s1 = torch.empty((R, T), dtype=torch.float64, device='cuda')
        n1 = torch.empty(R, dtype=torch.int32, device='cuda')
        c_h, s_h, n_h = np.empty((R, T)), np.empty((R, T)), np.empty(R, np.int32)

        def ar2(R=R, y=y, lam=lam, smin=smin, ws=ws2, c=c, s=s, n=n):
            L.dc_trace_deconv_ar2(y.data_ptr(), 0, T, R, T, g1, g2, H.data_ptr(), T + 1, lam.data_ptr(), smin.data_ptr(), None, ws.data_ptr(),
                                  c.data_ptr(), s.data_ptr(), n.data_ptr(), stream)

        def ar1(R=R, y=y, lam=lam, smin=smin, ws=ws1, c=c1, s=s1, n=n1):
            L.dc_trace_deconv_ar1(y.data_ptr(), 0, T, R, T, D, G.data_ptr(), lam.data_ptr(), smin.data_ptr(), ws.data_ptr(), c.data_ptr(),
                                  s.data_ptr(), n.data_ptr(), stream)

        def host(R=R, y_h=y_h, lam_h=lam_h, smin_h=smin_h, c_h=c_h, s_h=s_h, n_h=n_h):
            L.dc_trace_deconv_ar2_host(ptr(y_h), 0, T, R, T, g1, g2, ptr(H_h), T + 1, ptr(lam_h), ptr(smin_h), None, ptr(c_h), ptr(s_h), ptr(n_h))

        # what is timed is right: the device against the host entry point, every bit
        ar2()
        ar1()
        host()
        torch.cuda.synchronize()
        assert c.cpu().numpy().tobytes() == c_h.tobytes() and s.cpu().numpy().tobytes() == s_h.tobytes() and np.array_equal(n.cpu().numpy(), n_h)
        events, events1 = (s_h > 0).sum(1), (s1 > 0).sum(1).cpu().numpy()
        say('R = %d: device == host in every bit; AR(2) pools per trace median %d (max %d), events per trace median %d; AR(1) pools median %d, '
            'events median %d; median sigma_hat %.3f' % (R, int(np.median(n_h)), int(n_h.max()), int(np.median(events)),
                                                         int(np.median(n1.cpu().numpy())), int(np.median(events1)), float(np.median(smin_h)) / 2.0))
        rows += [(('ar2', R), 'dc_trace_deconv_ar2, %d traces' % R, ar2, True),
                 (('ar1', R), 'dc_trace_deconv_ar1, %d traces' % R, ar1, True),
                 (('host', R), 'dc_trace_deconv_ar2_host, one core, %d traces' % R, host, False)]

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
        two, one, host = (med[(k, R)][0] for k in ('ar2', 'ar1', 'host'))
        say('R = %d: AR(2) takes %.2f of AR(1) on the same traces and %.2f of its one-core host build (%s); %.2f us a frame, %.1f M samples/s'
            % (R, two / one, two / host, 'FASTER' if two < host else 'SLOWER', two * 1e3 / T, R * T / two / 1e3))
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
