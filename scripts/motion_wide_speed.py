"""Times of the wide (coarse-to-fine) shift search on one GPU (the figures of DESIGN.md section 4f, "Wide search").

    python scripts/motion_wide_speed.py [--hw 512] [--chunk 64] [--out FILE]

One chunk of `--chunk` int16 frames of `--hw` x `--hw`: a random scene cut at random offsets within +-S of each variant, plus noise.
Timed per chunk, for (S, c) = (16, 2), (16, 4), (32, 4), (64, 4), (128, 8): dc_motion_bin, the coarse dc_motion_ssd on the binned
frames, dc_motion_ssd_around and the two picks (dc_motion_pick on the coarse table + dc_motion_pick_around) -- beside the
exhaustive dc_motion_ssd at S = 16 and the H2D copy of the chunk out of pinned memory.  HIP events on the launch stream around 5
launches back to back; every row is warmed up once, then ONE run takes 5 rounds in which all rows are timed one after the other
(the variants interleaved, so that a drift of the clock meets all of them alike); the figure is the median of a row's 5 samples
(min - max).  The planted shifts of the chunk are compared with what each variant found.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = ((16, 2), (16, 4), (32, 4), (64, 4), (128, 8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hw', type=int, default=512)
    ap.add_argument('--chunk', type=int, default=64)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from deep_calcium_amd._lib import lib
    L = lib()
    H = W = args.hw
    C = args.chunk
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('wide search, one chunk of %d x %d x %d int16 (%.1f MB), %s' % (C, H, W, C * H * W * 2 / 1e6, torch.cuda.get_device_name(0)))
    stream = torch.cuda.current_stream().cuda_stream
    SM = max(S for S, _ in VARIANTS)
    rs = np.random.RandomState(0)
    scene = rs.randint(100, 1200, size=(H + 2 * SM, W + 2 * SM)).astype(np.int16)
    tmpl = scene[SM:SM + H, SM:SM + W].copy()
    dt = torch.from_numpy(tmpl).cuda()

    def chunk_at(S):
        """C frames cut within +-S, the four corners among them, plus noise -> (frames, offsets)."""
        offs = rs.randint(-S, S + 1, size=(C, 2))
        offs[:4] = [(S, S), (S, -S), (-S, S), (-S, -S)]
        raw = np.stack([scene[SM + a:SM + a + H, SM + b:SM + b + W] for a, b in offs])
        return raw + rs.randint(-30, 30, size=raw.shape).astype(np.int16), offs

    def timed(fn, reps=5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    rows, state = [], {}                                 # rows: (key, label, fn)
    raw16, offs16 = chunk_at(16)
    host = torch.from_numpy(raw16.copy()).pin_memory()
    dev16 = torch.empty((C, H, W), dtype=torch.int16, device='cuda')
    dev16.copy_(host)
    rows.append(('h2d', 'H2D copy of the chunk (pinned)', lambda: dev16.copy_(host, non_blocking=True)))
    full = torch.empty((C, 33, 33), dtype=torch.int64, device='cuda')
    full_shifts = torch.zeros((C, 2), dtype=torch.int32, device='cuda')
    rows.append(('full', 'exhaustive dc_motion_ssd, S = 16', lambda: L.dc_motion_ssd(dev16.data_ptr(), 0, C, dt.data_ptr(), H, W, 16, full.data_ptr(), stream)))
    for S, c in VARIANTS:
        Sc, Hc, Wc = -(-S // c), H // c, W // c
        raw, offs = (raw16, offs16) if S == 16 else chunk_at(S)
        st = dict(offs=offs, dev=dev16 if S == 16 else torch.from_numpy(raw).cuda(),
                  binned=torch.empty((C, Hc, Wc), dtype=torch.int16, device='cuda'), tb=torch.empty((Hc, Wc), dtype=torch.int16, device='cuda'),
                  cs=torch.empty((C, 2 * Sc + 1, 2 * Sc + 1), dtype=torch.int64, device='cuda'),
                  coarse=torch.zeros((C, 2), dtype=torch.int32, device='cuda'),
                  ws=torch.empty((C, 2 * c + 1, 2 * c + 1), dtype=torch.int64, device='cuda'),
                  shifts=torch.zeros((C, 2), dtype=torch.int32, device='cuda'))
        state[(S, c)] = st
        L.dc_motion_bin(dt.data_ptr(), 0, 1, H, W, c, st['tb'].data_ptr(), stream)

        def fns(S=S, c=c, Sc=Sc, Hc=Hc, Wc=Wc, st=st):
            d = st['dev'].data_ptr()
            return (('bin', lambda: L.dc_motion_bin(d, 0, C, H, W, c, st['binned'].data_ptr(), stream)),
                    ('coarse ssd', lambda: L.dc_motion_ssd(st['binned'].data_ptr(), 0, C, st['tb'].data_ptr(), Hc, Wc, Sc, st['cs'].data_ptr(), stream)),
                    ('window ssd', lambda: L.dc_motion_ssd_around(d, 0, C, dt.data_ptr(), H, W, S, c, st['coarse'].data_ptr(), c, st['ws'].data_ptr(), stream)),
                    ('picks', lambda: (L.dc_motion_pick(st['cs'].data_ptr(), C, Sc, st['coarse'].data_ptr(), None, stream),
                                       L.dc_motion_pick_around(st['ws'].data_ptr(), st['coarse'].data_ptr(), c, C, S, c, st['shifts'].data_ptr(), None, None,
                                                               stream))))
        for name, fn in fns():
            rows.append(((S, c, name), name, fn))
    # warm-up in pipeline order: every table a later row reads has been written
    for _, _, fn in rows:
        timed(fn, 1)
    L.dc_motion_pick(full.data_ptr(), C, 16, full_shifts.data_ptr(), None, stream)
    for S, c in VARIANTS:                                # the picks need the window table of the coarse picks just made
        st = state[(S, c)]
        L.dc_motion_ssd_around(st['dev'].data_ptr(), 0, C, dt.data_ptr(), H, W, S, c, st['coarse'].data_ptr(), c, st['ws'].data_ptr(), stream)
        L.dc_motion_pick_around(st['ws'].data_ptr(), st['coarse'].data_ptr(), c, C, S, c, st['shifts'].data_ptr(), None, None, stream)
    torch.cuda.synchronize()
    samples = dict((key, []) for key, _, _ in rows)
    for _ in range(5):                                   # one run, the variants interleaved
        for key, _, fn in rows:
            samples[key].append(timed(fn))
    med = dict((k, (float(np.median(v)), min(v), max(v))) for k, v in samples.items())
    h2d = med['h2d'][0]
    say('per chunk, 5 launches back to back per sample, median of 5 interleaved samples after a warm-up (min - max), and the ratio to the copy:')
    say('  %-36s %8.3f ms  (%.3f - %.3f)  %6.1f GB/s' % ((rows[0][1],) + med['h2d'] + (C * H * W * 2 / h2d / 1e6,)))
    say('  %-36s %8.3f ms  (%.3f - %.3f)  / H2D = %5.2f' % ((rows[1][1],) + med['full'] + (med['full'][0] / h2d,)))
    totals = {}
    for S, c in VARIANTS:
        total = 0.0
        for name in ('bin', 'coarse ssd', 'window ssd', 'picks'):
            ms, lo, hi = med[(S, c, name)]
            total += ms
            say('  S = %3d, c = %d  %-12s %8.3f ms  (%.3f - %.3f)  / H2D = %5.2f' % (S, c, name, ms, lo, hi, ms / h2d))
        totals[(S, c)] = total
        st = state[(S, c)]
        found = bool((st['shifts'].cpu().numpy() == -st['offs']).all())
        say('  S = %3d, c = %d  all four     %8.3f ms                     / H2D = %5.2f  (%s); planted shifts of the chunk recovered: %s'
            % (S, c, total, total / h2d, 'hides under the copy' if total < h2d else 'does NOT hide under the copy', found))
    say('exhaustive S = 16 found the planted shifts: %s' % bool((full_shifts.cpu().numpy() == -offs16).all()))
    for key in ((16, 2), (16, 4)):
        say('wide (%d, %d) / exhaustive S = 16 = %.3f  (%s)' % (key + (totals[key] / med['full'][0], 'faster' if totals[key] < med['full'][0] else 'NOT faster')))
    say('wide (64, 4) %s under the copy: %.3f ms against %.3f ms' % ('stays' if totals[(64, 4)] < h2d else 'does NOT stay', totals[(64, 4)], h2d))
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
