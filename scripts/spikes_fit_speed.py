"""Time of one UNet1D train step on one GPU (the figures DESIGN.md section 4e asks for).

    python scripts/spikes_fit_speed.py [--batch 20] [--frames 4096] [--nfb 32] [--steps 10] [--cpu-steps 1] [--out FILE]

A freshly initialised model, random z-scored windows and sparse random labels; nothing is read from disk.  Timed:
 (a) UNet1DTrainEngine.forward_backward + adam_step, launched from Python: HIP events around `--steps` steps after two warm-up
     steps, the median of 5 such samples;
 (b) a float32 torch-CPU restatement of the same step on this host (training-mode F.batch_norm, autograd, torch.optim.Adam),
     `--cpu-steps` steps timed after one warm-up step.  No dropout in either (prop_dropout_base 0): the CPU side has no
     matching RNG, and the masks cost the device nothing measurable.
The last line printed is one JSON object with all of it.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_cpu_step(torch, W, opt, x, y, margin):
    F = torch.nn.functional

    def conv_layer(h, i):
        k, b, ga, be = W[4 * i:4 * i + 4]
        return F.relu(F.batch_norm(F.conv1d(h, k, b, padding=2), None, None, ga, be, training=True, eps=1e-3))

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
    pool = margin + 1
    l = F.pad(F.conv1d(h, W[-2], W[-1]), ((pool - 1) // 2, pool // 2), value=float('-inf'))
    p = torch.softmax(F.max_pool1d(l, pool, 1), dim=1)[:, -1, :]
    loss = (-(2. * y * torch.log(p + 1e-7) + (1. - y) * torch.log(1. - p + 1e-7))).mean()
    opt.zero_grad()
    loss.backward()
    opt.step()
    return float(loss.detach())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=20)
    ap.add_argument('--frames', type=int, default=4096)
    ap.add_argument('--nfb', type=int, default=32)
    ap.add_argument('--margin', type=int, default=4)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--cpu-steps', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()

    import torch
    from deep_calcium_amd.unet1d_train import UNet1DTrainEngine
    rs = np.random.RandomState(0)
    x = rs.randn(a.batch, a.frames).astype(np.float32)
    y = (rs.uniform(size=(a.batch, a.frames)) < 0.05).astype(np.uint8)
    res = dict(batch=a.batch, frames=a.frames, nfb=a.nfb, margin=a.margin, device=None)

    eng = UNet1DTrainEngine((a.frames,), nb_filters_base=a.nfb, prop_dropout_base=0., margin=a.margin)
    res['device'] = torch.cuda.get_device_name(eng.device)
    xd, yd = torch.from_numpy(x).to(eng.device), torch.from_numpy(y).to(eng.device)

    def step():
        eng.forward_backward(xd, yd)
        eng.adam_step(0.002)

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    samples = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        samples.append(e0.elapsed_time(e1) / a.steps)
    res['device_step_ms'] = dict(median=float(np.median(samples)), min=float(min(samples)), max=float(max(samples)))
    res['device_loss'] = float(eng.read_sums()[0] / (a.batch * a.frames))
    print('device: %.3f ms per train step (%.3f - %.3f)' % (np.median(samples), min(samples), max(samples)))

    if a.cpu_steps > 0:
        W = []
        for i, w in enumerate(UNet1DTrainEngine((a.frames,), nb_filters_base=a.nfb, prop_dropout_base=0., margin=a.margin).get_weights()):
            if i % 6 < 4 or i >= 108:
                t = torch.from_numpy(w)
                W.append((t.permute(2, 1, 0).contiguous() if t.dim() == 3 else t).requires_grad_(True))
        opt = torch.optim.Adam(W, lr=0.002, eps=1e-8)
        xc, yc = torch.from_numpy(x), torch.from_numpy(y.astype(np.float32))
        torch_cpu_step(torch, W, opt, xc, yc, a.margin)
        t0 = time.perf_counter()
        for _ in range(a.cpu_steps):
            cpu_loss = torch_cpu_step(torch, W, opt, xc, yc, a.margin)
        cpu_ms = (time.perf_counter() - t0) * 1e3 / a.cpu_steps
        res['cpu_step_ms'], res['cpu_threads'], res['cpu_loss'] = cpu_ms, torch.get_num_threads(), cpu_loss
        res['cpu_over_device'] = cpu_ms / res['device_step_ms']['median']
        print('torch CPU (%d threads): %.1f ms per train step, %.0f x the device' % (torch.get_num_threads(), cpu_ms, res['cpu_over_device']))

    line = json.dumps(res)
    if a.out:
        with open(a.out, 'w') as fp:
            fp.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
