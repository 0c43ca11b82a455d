"""Times of the bidirectional scan-phase correction on one GPU (the figures of DESIGN.md section 4f, "Scan-phase offset").

    python scripts/bidi_speed.py [--hw 512] [--chunk 64] [--out FILE]

One chunk of `--chunk` int16 frames of `--hw` x `--hw`: a random scene plus noise, the odd lines cut at a planted offset of 3.
Timed per chunk: dc_bidi_scores at P = 4, 8 and 16 and dc_bidi_apply -- beside the H2D copy of the chunk out of pinned memory,
dc_motion_apply and dc_motion_ssd at S = 4 on the same chunk.  HIP events on the launch stream around 5 launches back to back;
every row is warmed up once, then ONE run takes 5 rounds in which all rows are timed one after the other (the variants interleaved,
so that a drift of the clock meets all of them alike); the figure is the median of a row's 5 samples (min - max).  The planted
offset is compared with what each radius found.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RADII = (4, 8, 16)
PLANTED = 3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hw', type=int, default=512)
    ap.add_argument('--chunk', type=int, default=64)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from deep_calcium_amd._lib import lib
    from deep_calcium_amd.motion import pick_bidi
    L = lib()
    H = W = args.hw
    C = args.chunk
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('scan-phase offset, one chunk of %d x %d x %d int16 (%.1f MB), %s' % (C, H, W, C * H * W * 2 / 1e6, torch.cuda.get_device_name(0)))
    stream = torch.cuda.current_stream().cuda_stream
    rs = np.random.RandomState(0)
    M = max(RADII)
    # a smooth scene (a random field summed over 5 x 5 neighbourhoods), so that neighbouring lines agree where they are aligned
    field = rs.randint(0, 80, size=(H + 4, W + 2 * M + 4)).astype(np.int64)
    scene = sum(field[i:i + H, j:j + W + 2 * M] for i in range(5) for j in range(5)) + 100
    raw = np.empty((C, H, W), np.int16)
    for t in range(C):
        full = scene + rs.randint(-30, 30, size=scene.shape)
        raw[t] = full[:, M:M + W]
        raw[t, 1::2] = full[1::2, M + PLANTED:M + PLANTED + W]
    tmpl = scene[:, M:M + W].astype(np.int16)

    def timed(fn, reps=5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    host = torch.from_numpy(raw.copy()).pin_memory()
    dev = torch.empty((C, H, W), dtype=torch.int16, device='cuda')
    dev.copy_(host)
    out = torch.empty((C, H, W), dtype=torch.int16, device='cuda')
    dt = torch.from_numpy(tmpl).cuda()
    shifts = torch.zeros((C, 2), dtype=torch.int32, device='cuda')
    ssd = torch.empty((C, 9, 9), dtype=torch.int64, device='cuda')
    tables = dict((P, torch.empty((C, 2 * P + 1), dtype=torch.int64, device='cuda')) for P in RADII)
    rows = [('h2d', 'H2D copy of the chunk (pinned)', lambda: dev.copy_(host, non_blocking=True))]
    for P in RADII:
        rows.append((('scores', P), 'dc_bidi_scores, P = %d' % P,
                     lambda P=P: L.dc_bidi_scores(dev.data_ptr(), 0, C, H, W, P, tables[P].data_ptr(), stream)))
    rows.append(('apply', 'dc_bidi_apply', lambda: L.dc_bidi_apply(dev.data_ptr(), C, -PLANTED, H, W, 0, out.data_ptr(), stream)))
    rows.append(('move', 'dc_motion_apply', lambda: L.dc_motion_apply(dev.data_ptr(), C, shifts.data_ptr(), H, W, 0, out.data_ptr(), stream)))
    rows.append(('ssd', 'dc_motion_ssd, S = 4', lambda: L.dc_motion_ssd(dev.data_ptr(), 0, C, dt.data_ptr(), H, W, 4, ssd.data_ptr(), stream)))
    for _, _, fn in rows:                                # warm-up
        timed(fn, 1)
    samples = dict((key, []) for key, _, _ in rows)
    for _ in range(5):                                   # one run, the variants interleaved
        for key, _, fn in rows:
            samples[key].append(timed(fn))
    med = dict((k, (float(np.median(v)), min(v), max(v))) for k, v in samples.items())
    h2d = med['h2d'][0]
    say('per chunk, 5 launches back to back per sample, median of 5 interleaved samples after a warm-up (min - max), and the ratio to the copy:')
    say('  %-32s %8.3f ms  (%.3f - %.3f)  %6.1f GB/s' % ((rows[0][1],) + med['h2d'] + (C * H * W * 2 / h2d / 1e6,)))
    for key, label, _ in rows[1:]:
        ms, lo, hi = med[key]
        say('  %-32s %8.3f ms  (%.3f - %.3f)  / H2D = %5.2f  (%s)' % (label, ms, lo, hi, ms / h2d,
                                                                  'under the copy' if ms < h2d else 'NOT under the copy'))
    for P in RADII:
        sc = tables[P].cpu().numpy()
        totals = [sum(int(v) for v in sc[:, k]) for k in range(2 * P + 1)]
        say('P = %2d found the offset %+d (planted: odd lines cut at %+d, so %+d)' % (P, pick_bidi(totals), PLANTED, -PLANTED))
    both = med[('scores', 8)][0] + med['apply'][0]
    say('scores at P = 8 + apply = %.3f ms: %s under the copy of %.3f ms' % (both, 'stays' if both < h2d else 'does NOT stay', h2d))
    say('dc_bidi_scores at P = 16 %s under the copy' % ('stays' if med[('scores', 16)][0] < h2d else 'does NOT stay'))
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
