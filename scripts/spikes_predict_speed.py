"""Times of the UNet1D spike inference on one GPU (the figures of DESIGN.md section 4d).

    python scripts/spikes_predict_speed.py [--traces 300] [--frames 8192] [--nfb 32] [--batch 300] [--cpu-traces 32] [--out FILE]

A random model (He-normal kernels) and random z-scored traces; nothing is read from disk.  Timed:
 (a) kernel time of every launch of one forward at (batch, frames): HIP events on the launch stream around 5 launches back to
     back, median of 5 such samples after a warm-up, with the layer's FLOPs, TFLOP/s and the fraction of the 157 TFLOP/s
     fp32-matrix peak for the implicit-GEMM layers;
 (b) the whole forward (UNet1DEngine.forward, launched from Python) over all traces in chunks of `batch`, events around it;
 (c) a torch-CPU float32 forward of the same network on this host (F.conv1d / F.batch_norm / F.max_pool1d), `--cpu-traces`
     traces timed once after a warm-up and scaled to all traces.
The last line printed is one JSON object with all of it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_TFLOPS = 157.3                 # MI355X fp32 matrix (v_mfma_f32_32x32x2_f32), vendor figure


def random_model(nfb, seed=0):
    from deep_calcium_amd.unet1d import conv_plan
    rs = np.random.RandomState(seed)
    w = []
    for cin, cout in conv_plan(nfb):
        w += [rs.randn(5, cin, cout) * np.sqrt(2. / (5 * cin)), 0.05 * rs.randn(cout), 1. + 0.1 * rs.randn(cout), 0.1 * rs.randn(cout),
              0.1 * rs.randn(cout), rs.uniform(0.5, 1.5, cout)]
    w += [rs.randn(1, nfb, 2) * np.sqrt(2. / nfb) * 0.07, 0.05 * rs.randn(2)]
    return [a.astype(np.float32) for a in w]


def torch_cpu_forward(torch, W, x, margin):
    F = torch.nn.functional

    def conv_layer(h, i):
        k, b, ga, be, mm, mv = W[6 * i:6 * i + 6]
        return F.relu(F.batch_norm(F.conv1d(h, k, b, padding=2), mm, mv, ga, be, training=False, eps=1e-3))

    h = x[:, None, :]
    skips, k = [], 0
    for lvl in range(5):
        if lvl:
            h = F.max_pool1d(h, 2, 2)
        h = conv_layer(conv_layer(h, k), k + 1)
        k += 2
        if lvl < 4:
            skips.append(h)
    for lvl in (3, 2, 1, 0):
        h = torch.cat([h.repeat_interleave(2, dim=2), skips[lvl]], dim=1)
        h = conv_layer(conv_layer(h, k), k + 1)
        k += 2
    l = F.max_pool1d(F.conv1d(h, W[108], W[109]), margin + 1, 1, padding=margin // 2)
    return torch.softmax(l, dim=1)[:, -1, :]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--traces', type=int, default=300)
    ap.add_argument('--frames', type=int, default=8192)
    ap.add_argument('--nfb', type=int, default=32)
    ap.add_argument('--batch', type=int, default=300)
    ap.add_argument('--cpu-traces', type=int, default=32)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from deep_calcium_amd import UNet1DEngine
    R, T, nfb, B, margin = args.traces, args.frames, args.nfb, min(args.batch, args.traces), 4
    weights = random_model(nfb)
    eng = UNet1DEngine(weights, nfb, margin)
    x = torch.randn(R, T, device='cuda')
    res = dict(device=torch.cuda.get_device_name(0), traces=R, frames=T, nfb=nfb, batch=B, peak_tflops=PEAK_TFLOPS)
    print('UNet1D forward, %d traces x %d samples, nfb %d, batch %d, %s' % (R, T, nfb, B, res['device']), flush=True)

    def timed(fn, reps=1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    # ---- (a) per launch: record one forward's launches, then replay each alone on the buffers that forward left behind
    L = eng.L
    L.record_begin()
    eng.forward(x[:B])
    ops = L.record_end()
    torch.cuda.synchronize()
    layers, total_ms, total_flop = [], 0., 0.
    for name, a in ops:
        fn = getattr(L, name)
        timed(lambda: fn(*a), 5)
        ms = float(np.median([timed(lambda: fn(*a), 5) for _ in range(5)]))
        flop = 0.
        if name == 'dc_conv1d_k5_fwd':
            n, t, ci, co = a[7:11]
            flop = 2. * n * t * 5 * ci * co
            what = '%4d -> %4d ch x %5d samples' % (ci, co, t)
        elif name == 'dc_conv1d_k5_c1_fwd':
            n, t, co = a[7:10]
            flop = 2. * n * t * 5 * co
            what = '   1 -> %4d ch x %5d samples' % (co, t)
        else:
            what = ''
        tf = flop / ms / 1e9
        row = dict(launch=name, what=what.strip(), ms=round(ms, 4), gflop=round(flop / 1e9, 2), tflops=round(tf, 2))
        if name == 'dc_conv1d_k5_fwd':
            row['of_peak'] = round(tf / PEAK_TFLOPS, 3)
        layers.append(row)
        total_ms += ms
        total_flop += flop
        print('  %-22s %-32s %8.3f ms %9.1f GFLOP %7.2f TFLOP/s%s'
              % (name, what, ms, flop / 1e9, tf, '  %4.1f %% of peak' % (100 * tf / PEAK_TFLOPS) if 'of_peak' in row else ''), flush=True)
    dom = max(layers, key=lambda r: r['ms'])
    res.update(layers=layers, kernels_ms=round(total_ms, 3), gflop_per_batch=round(total_flop / 1e9, 1),
               dominant=dict(launch=dom['launch'], what=dom['what'], ms=dom['ms'], of_peak=dom.get('of_peak')))
    print('  sum of the %d launches %8.3f ms = %.2f TFLOP/s overall; dominant: %s %s' % (len(ops), total_ms, total_flop / total_ms / 1e9,
                                                                                      dom['launch'], dom['what']), flush=True)

    # ---- (b) the whole forward over all traces, launched from Python
    def forward_all():
        for a in range(0, R, B):
            eng.forward(x[a:a + B])
    timed(forward_all)
    samples = [timed(forward_all) for _ in range(5)]
    res.update(forward_ms=round(float(np.median(samples)), 3), forward_ms_min=round(min(samples), 3), forward_ms_max=round(max(samples), 3))
    print('(b) forward of all %d traces: %.3f ms (%.3f - %.3f)' % (R, res['forward_ms'], min(samples), max(samples)), flush=True)

    # ---- (c) torch-CPU float32 on this host
    n = max(1, min(args.cpu_traces, R))
    W = [torch.from_numpy(a) for a in weights]
    for i in list(range(0, 108, 6)) + [108]:
        W[i] = W[i].permute(2, 1, 0).contiguous()
    xc = x[:n].cpu()
    with torch.no_grad():
        pc = torch_cpu_forward(torch, W, xc[:1], margin)
        t0 = time.perf_counter()
        pc = torch_cpu_forward(torch, W, xc, margin)
        cpu_s = time.perf_counter() - t0
    diff = float((eng.forward(x[:n]).cpu() - pc).abs().max())
    res.update(cpu_traces=n, cpu_threads=torch.get_num_threads(), cpu_s=round(cpu_s, 3), cpu_s_scaled=round(cpu_s * R / n, 2),
               max_abs_diff_vs_cpu=diff)
    print('(c) torch-CPU float32, %d threads: %d traces in %.3f s -> %.1f s for all %d; max |p_gpu - p_cpu| = %.2g'
          % (res['cpu_threads'], n, cpu_s, cpu_s * R / n, R, diff), flush=True)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write(line + '\n')


if __name__ == '__main__':
    main()
