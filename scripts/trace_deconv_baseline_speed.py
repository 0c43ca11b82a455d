"""Times of the joint search of the threshold and the baseline on one GPU (the figures of DESIGN.md section 4q and of the README's
"A baseline in the deconvolution").

    python scripts/trace_deconv_baseline_speed.py [--frames 8192] [--rois 512,4096] [--rounds 24] [--out FILE]

The setup of scripts/trace_deconv_search_speed.py: the traces of the reach table (sigma 0.3) as a fluorescence, dc_trace_baseline
turns them into the float32 dF/F that lies on the device, g = exp(-1/8), sigma = dc_trace_noise's sigma_hat.  Timed per trace count,
by HIP events on the launch stream: dc_trace_deconv_ar1_constrained_base (s_min and the baseline searched jointly from b_0 = 0,
`rounds` rounds; workspace, state and outputs allocated once), beside it dc_trace_deconv_ar1_constrained of the same library on the
same traces (no baseline: what the cost is measured against), and ONE launch of the residual kernel by itself
(dc_trace_deconv_base_step in the fit mode on the stacks the joint call left).  The joint call enqueues 2 N + 2 forward passes where
the plain one enqueues N + 2: the expected ratio at 24 rounds is 50 / 26 = 1.92.  Every row is warmed up once, then ONE run takes 5
rounds in which the rows are timed one after the other (the variants interleaved, so that a drift of the clock meets all of them
alike); the figure is the median of a row's samples (min - max).  Before anything is timed the joint result is compared with
dc_trace_deconv_ar1_constrained_base_host's in every bit.
"""
import argparse
import ctypes
import os
import sys

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

    say('joint search of s_min and the baseline, %d rounds, traces of %d frames, %s' % (N, T, torch.cuda.get_device_name(0)))
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
        zero = torch.from_numpy(zero_h).cuda()
        ws = torch.empty(L.dc_trace_deconv_ws_bytes(R, T) // 8, dtype=torch.float64, device='cuda')
        state = torch.empty(L.dc_trace_deconv_base_state_bytes(R) // 8, dtype=torch.float64, device='cuda')
        c = torch.empty((R, T), dtype=torch.float64, device='cuda')
        s = torch.empty((R, T), dtype=torch.float64, device='cuda')
        n = torch.empty(R, dtype=torch.int32, device='cuda')
        param, rss, base = (torch.empty(R, dtype=torch.float64, device='cuda') for _ in range(3))
        status = torch.empty(R, dtype=torch.int32, device='cuda')
        scratch = torch.zeros(R, dtype=torch.float64, device='cuda')
        c_h, s_h, n_h = np.empty((R, T)), np.empty((R, T)), np.empty(R, np.int32)
        param_h, rss_h, base_h, status_h = np.empty(R), np.empty(R), np.zeros(R), np.empty(R, np.int32)

        def joint(R=R, dff=dff, sigma=sigma, zero=zero, ws=ws, state=state, c=c, s=s, n=n, param=param, base=base, rss=rss, status=status):
            base.zero_()                                               # b_0 = 0: the call reads it
            L.dc_trace_deconv_ar1_constrained_base(dff.data_ptr(), 0, T, R, T, g, None, G.data_ptr(), 0, 0, sigma.data_ptr(), zero.data_ptr(), N,
                                                   ws.data_ptr(), state.data_ptr(), c.data_ptr(), s.data_ptr(), n.data_ptr(), param.data_ptr(),
                                                   base.data_ptr(), rss.data_ptr(), status.data_ptr(), stream)

        def plain(R=R, dff=dff, sigma=sigma, zero=zero, ws=ws, state=state, c=c, s=s, n=n, param=param, rss=rss, status=status):
            L.dc_trace_deconv_ar1_constrained(dff.data_ptr(), 0, T, R, T, g, None, G.data_ptr(), 0, 0, sigma.data_ptr(), zero.data_ptr(), N,
                                              ws.data_ptr(), state.data_ptr(), c.data_ptr(), s.data_ptr(), n.data_ptr(), param.data_ptr(),
                                              rss.data_ptr(), status.data_ptr(), stream)

        def step(R=R, dff=dff, ws=ws, n=n, scratch=scratch):
            # the stacks of the call before it; the fit mode needs no state, its baseline goes to scratch
            L.dc_trace_deconv_base_step(dff.data_ptr(), 0, T, R, T, G.data_ptr(), 0, ws.data_ptr(), n.data_ptr(), 0, None, None, scratch.data_ptr(),
                                        None, None, None, stream)

        # what is timed is right: the device against the host entry point, every bit
        joint()
        L.dc_trace_deconv_ar1_constrained_base_host(ptr(dff_h), 0, T, R, T, ptr(G_h), 0, 0, ptr(sigma_h), ptr(zero_h), N, ptr(c_h), ptr(s_h), ptr(n_h),
                                                    ptr(param_h), ptr(base_h), ptr(rss_h), ptr(status_h))
        torch.cuda.synchronize()
        for a, b in ((c, c_h), (s, s_h), (n, n_h), (param, param_h), (base, base_h), (rss, rss_h), (status, status_h)):
            assert a.cpu().numpy().tobytes() == b.tobytes()
        events = int((s_h > 0).sum())
        plain()
        torch.cuda.synchronize()
        ratio, b_ratio = param_h / sigma_h, base_h / sigma_h
        say('R = %d: device == host in every bit; s_min / sigma_hat found min / median / max = %.2f / %.2f / %.2f, baseline / sigma_hat = '
            '%.2f / %.2f / %.2f, status 0 / 1 / 2 = %d / %d / %d, events %d (without a baseline: %d)'
            % (R, ratio.min(), np.median(ratio), ratio.max(), b_ratio.min(), np.median(b_ratio), b_ratio.max(), (status_h == 0).sum(),
               (status_h == 1).sum(), (status_h == 2).sum(), events, int((s > 0).sum().item())))
        keep.append((num, dff, sigma, zero, ws, state, c, s, n, param, base, rss, status, scratch))
        rows += [(('joint', R), 'dc_trace_deconv_ar1_constrained_base, %d rounds, %d traces' % (N, R), joint),
                 (('step', R), 'one dc_trace_deconv_base_step launch, %d traces' % R, step),
                 (('plain', R), 'dc_trace_deconv_ar1_constrained, %d rounds, %d traces' % (N, R), plain)]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    for _, _, fn in rows:                                # warm-up
        timed(fn)
    samples = dict((key, []) for key, _, _ in rows)
    for i in range(5):                                   # one run, the variants interleaved
        for key, _, fn in rows:
            samples[key].append(timed(fn))
    med = dict((k, (float(np.median(v)), min(v), max(v))) for k, v in samples.items())
    say('per call, one call per sample, median of 5 interleaved samples after a warm-up (min - max):')
    for key, label, _ in rows:
        ms, lo, hi = med[key]
        say('  %-72s %10.3f ms  (%.3f - %.3f)' % (label, ms, lo, hi))
    for R in counts:
        joint, step, plain = (med[(k, R)][0] for k in ('joint', 'step', 'plain'))
        say('R = %d: joint / plain = %.2f (expected (2 N + 2) / (N + 2) = %.2f); the %d residual launches are %.2f of the joint call'
            % (R, joint / plain, (2 * N + 2) / (N + 2.0), 2 * N + 1, (2 * N + 1) * step / joint))
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
