"""Times of the noise-constrained search on one GPU (the figures of DESIGN.md section 4p and of the README's "Choosing the threshold
by the noise").

    python scripts/trace_deconv_search_speed.py [--frames 8192] [--rois 512,4096] [--rounds 24] [--out FILE]

The setup of scripts/trace_deconv_speed.py: the traces of the reach table (sigma 0.3) as a fluorescence, dc_trace_baseline turns
them into the float32 dF/F that lies on the device, g = exp(-1/8).  Timed per trace count: dc_trace_deconv_ar1_constrained (s_min
searched, `rounds` rounds, sigma = dc_trace_noise's sigma_hat; workspace, state and outputs allocated once), ONE residual-and-step
launch by itself (dc_trace_deconv_search_step on the stacks the call left), dc_trace_deconv_ar1 on the same traces at
s_min = 3 sigma_hat -- a single pass, what the cost is measured against -- by HIP events on the launch stream, and
dc_trace_deconv_ar1_constrained_host on ONE core of the same box by the wall clock.  Every row is warmed up once, then ONE run takes
5 rounds in which the rows are timed one after the other (the variants interleaved, so that a drift of the clock meets all of them
alike; the host rows, seconds each, in rounds 0, 2 and 4 only); the figure is the median of a row's samples (min - max).  Before
anything is timed the device result is compared with the host entry point's in every bit.
"""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from trace_deconv_speed import traces      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8192)
    ap.add_argument('--rois', default='512,4096')
    ap.add_argument('--rounds', type=int, default=24)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from deep_calcium_amd._lib import lib
    from deep_calcium_amd.deconv import ar1_table
    L = lib()
    T, N = args.frames, args.rounds
    counts = [int(v) for v in args.rois.split(',')]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('noise-constrained search of s_min, %d rounds, traces of %d frames, %s; host: one core' % (N, T, torch.cuda.get_device_name(0)))
    stream = torch.cuda.current_stream().cuda_stream
    g = float(np.exp(-1.0 / 8.0))
    G_h = ar1_table(g, T)
    G = torch.from_numpy(G_h).cuda()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)                  # noqa: E731
    y_all = traces(max(counts), T)
    rows, keep = [], []
    for R in counts:
        num = torch.from_numpy(np.rint(4000.0 * (1.0 + y_all[:R].astype(np.float64))).astype(np.int64)).cuda()
        dff = torch.empty((R, T), dtype=torch.float32, device='cuda')
        L.dc_trace_baseline(num.data_ptr(), T, R, T, 900, 8, None, dff.data_ptr(), stream)
        sigma = torch.empty(R, dtype=torch.float64, device='cuda')
        L.dc_trace_noise(dff.data_ptr(), 0, T, R, T, sigma.data_ptr(), stream)
        dff_h, sigma_h = dff.cpu().numpy(), sigma.cpu().numpy()
        zero_h = np.zeros(R)
        zero, smin3 = torch.from_numpy(zero_h).cuda(), torch.from_numpy(3.0 * sigma_h).cuda()
        ws = torch.empty(L.dc_trace_deconv_ws_bytes(R, T) // 8, dtype=torch.float64, device='cuda')
        state = torch.empty(L.dc_trace_deconv_search_state_bytes(R) // 8, dtype=torch.float64, device='cuda')
        c = torch.empty((R, T), dtype=torch.float64, device='cuda')
        s = torch.empty((R, T), dtype=torch.float64, device='cuda')
        n = torch.empty(R, dtype=torch.int32, device='cuda')
        param, rss = torch.empty(R, dtype=torch.float64, device='cuda'), torch.empty(R, dtype=torch.float64, device='cuda')
        status = torch.empty(R, dtype=torch.int32, device='cuda')
        scratch, scratch_i = torch.zeros((2, R), dtype=torch.float64, device='cuda'), torch.empty(R, dtype=torch.int32, device='cuda')
        c_h, s_h, n_h = np.empty((R, T)), np.empty((R, T)), np.empty(R, np.int32)
        param_h, rss_h, status_h = np.empty(R), np.empty(R), np.empty(R, np.int32)

        def search(R=R, dff=dff, sigma=sigma, zero=zero, ws=ws, state=state, c=c, s=s, n=n, param=param, rss=rss, status=status):
            L.dc_trace_deconv_ar1_constrained(dff.data_ptr(), 0, T, R, T, g, None, G.data_ptr(), 0, 0, sigma.data_ptr(), zero.data_ptr(), N,
                                              ws.data_ptr(), state.data_ptr(), c.data_ptr(), s.data_ptr(), n.data_ptr(), param.data_ptr(),
                                              rss.data_ptr(), status.data_ptr(), stream)

        def step(R=R, dff=dff, ws=ws, state=state, n=n, scratch=scratch, scratch_i=scratch_i):
            # the stacks of the last search; the step's outputs go to scratch, the state words it moves are rewritten by the next search
            L.dc_trace_deconv_search_step(dff.data_ptr(), 0, T, R, T, G.data_ptr(), 0, ws.data_ptr(), n.data_ptr(), 1, state.data_ptr(),
                                          scratch[0].data_ptr(), scratch[1].data_ptr(), scratch_i.data_ptr(), stream)

        def single(R=R, dff=dff, zero=zero, smin3=smin3, ws=ws, c=c, s=s, n=n):
            L.dc_trace_deconv_ar1(dff.data_ptr(), 0, T, R, T, g, G.data_ptr(), zero.data_ptr(), smin3.data_ptr(), ws.data_ptr(), c.data_ptr(),
                                  s.data_ptr(), n.data_ptr(), stream)

        def host(R=R, dff_h=dff_h, sigma_h=sigma_h, zero_h=zero_h, c_h=c_h, s_h=s_h, n_h=n_h, param_h=param_h, rss_h=rss_h, status_h=status_h):
            L.dc_trace_deconv_ar1_constrained_host(ptr(dff_h), 0, T, R, T, ptr(G_h), 0, ptr(sigma_h), ptr(zero_h), N, ptr(c_h), ptr(s_h), ptr(n_h),
                                                   ptr(param_h), ptr(rss_h), ptr(status_h))

        # what is timed is right: the device against the host entry point, every bit
        search()
        host()
        torch.cuda.synchronize()
        for a, b in ((c, c_h), (s, s_h), (n, n_h), (param, param_h), (rss, rss_h), (status, status_h)):
            assert a.cpu().numpy().tobytes() == b.tobytes()
        ratio = param_h / sigma_h
        say('R = %d: device == host in every bit; s_min / sigma_hat found min / median / max = %.2f / %.2f / %.2f, status 0 / 1 / 2 = %d / %d / %d, '
            'pools per trace at p* median %d, median sigma_hat %.3f' % (R, ratio.min(), np.median(ratio), ratio.max(), (status_h == 0).sum(),
                                                                         (status_h == 1).sum(), (status_h == 2).sum(), int(np.median(n_h)),
                                                                         float(np.median(sigma_h))))
        keep.append((num, dff, sigma, zero, smin3, ws, state, c, s, n, param, rss, status, scratch, scratch_i))
        # `step` follows `search` in every round: the stacks it reads are those of the final pass at p*
        rows += [(('search', R), 'dc_trace_deconv_ar1_constrained, %d rounds, %d traces' % (N, R), search, True),
                 (('step', R), 'one residual-and-step launch, %d traces' % R, step, True),
                 (('single', R), 'dc_trace_deconv_ar1 (one pass, s_min = 3 sigma_hat), %d traces' % R, single, True),
                 (('host', R), 'dc_trace_deconv_ar1_constrained_host, one core, %d traces' % R, host, False)]

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

    for _, _, fn, on_gpu in rows:                        # warm-up (the host rows ran in the comparison above)
        if on_gpu:
            timed(fn, on_gpu)
    samples = dict((key, []) for key, _, _, _ in rows)
    for i in range(5):                                   # one run, the variants interleaved
        for key, _, fn, on_gpu in rows:
            if on_gpu or i % 2 == 0:
                samples[key].append(timed(fn, on_gpu))
    med = dict((k, (float(np.median(v)), min(v), max(v))) for k, v in samples.items())
    say('per call, one call per sample, median of 5 interleaved samples (host: 3) after a warm-up (min - max):')
    for key, label, _, _ in rows:
        ms, lo, hi = med[key]
        say('  %-72s %10.3f ms  (%.3f - %.3f)' % (label, ms, lo, hi))
    for R in counts:
        search, step, single, host = (med[(k, R)][0] for k in ('search', 'step', 'single', 'host'))
        say('R = %d: constrained / single pass = %.1f (expected about rounds + 2 = %d); the %d residual-and-step launches are %.2f of the '
            'constrained call; one of them takes %.2f of a single pass (forward + fill); the device takes %.3f of the one-core host build (%s)'
            % (R, search / single, N + 2, N + 1, (N + 1) * step / search, step / single, search / host, 'FASTER' if search < host else 'SLOWER'))
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
