"""Times of the motion-correction path on one GPU (the figures of DESIGN.md section 4f).

    python scripts/motion_correct_speed.py [--frames 3000] [--hw 512] [--chunk 64] [--blocks 4x4] [--max-dev 3] [--out FILE]

A synthetic int16 recording -- a random scene cut at random offsets within +-5 pixels, plus noise -- is written as an .npz next to
the output (np.savez: stored, so it is memory-mapped).  Timed, for max_shift S = 4, 8 and 16 and chunks of `--chunk` frames:
 (a) the H2D copy of one chunk out of pinned memory;
 (b) kernel time per chunk of dc_motion_ssd, dc_motion_pick and dc_motion_apply: HIP events on the launch stream around 5 launches
     back to back, median of 5 such samples after a warm-up (min - max), and the ratio of each to the copy; then the same for the
     piecewise-rigid entry points dc_motion_block_ssd, dc_motion_block_pick and dc_motion_warp at `--blocks` and `--max-dev`,
     on the rigid shifts just found; then the sub-pixel entry points: dc_motion_refine and dc_motion_block_refine on those tables,
     dc_motion_apply_sub at fine shifts with both fractions non-zero (two source rows, nine values each) and dc_motion_warp_sub
     at equal fine block shifts (every group of 8 shares its split) and at block shifts a few sixteenths apart (the field changes
     within most groups: value by value);
 (c) wall time of estimate_shifts_device over the whole recording with a given template (median of 5 after a warm-up, page cache
     warm), and whether the planted shifts came back;
 (d) a numpy restatement of the same search on a few frames, scaled to a chunk.
"""
import argparse
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_of(fn, n=5, warm=1):
    for _ in range(warm):
        fn()
    return float(np.median([fn() for _ in range(n)]))


def numpy_scores(frames, tmpl, S):
    T, H, W = frames.shape
    t = tmpl[S:H - S, S:W - S].astype(np.int64)
    f = frames.astype(np.int64)
    out = np.zeros((T, 2 * S + 1, 2 * S + 1), np.int64)
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            d = t[None] - f[:, S + dy:H - S + dy, S + dx:W - S + dx]
            out[:, dy + S, dx + S] = (d * d).sum(axis=(1, 2))
    return out


def rs_blocks(C, By, Bx):
    """Per-block offsets within +-6 sixteenths: block shifts as far apart as a refinement leaves them."""
    return np.random.RandomState(1).randint(-6, 7, size=(C, By, Bx, 2)).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=3000)
    ap.add_argument('--hw', type=int, default=512)
    ap.add_argument('--chunk', type=int, default=64)
    ap.add_argument('--host-frames', type=int, default=2, help='frames of the numpy search (the time is scaled to a chunk)')
    ap.add_argument('--blocks', default='4x4', help='the block grid ByxBx of the piecewise-rigid rows')
    ap.add_argument('--max-dev', type=int, default=3, help='their deviation radius D')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from deep_calcium_amd import estimate_shifts_device
    from deep_calcium_amd._lib import lib
    L = lib()
    T, H, W, C = args.frames, args.hw, args.hw, args.chunk
    By, Bx = (int(v) for v in args.blocks.lower().split('x'))
    D = args.max_dev
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('motion correction, %d x %d x %d int16 (%.2f GB), chunks of %d frames, %s'
        % (T, H, W, T * H * W * 2 / 1e9, C, torch.cuda.get_device_name(0)))
    rs = np.random.RandomState(0)
    M = 5
    scene = rs.randint(100, 1200, size=(H + 2 * M, W + 2 * M)).astype(np.int16)
    offs = rs.randint(-M, M + 1, size=(T, 2))
    raw = np.empty((T, H, W), np.int16)
    for t in range(T):
        raw[t] = scene[M + offs[t, 0]:M + offs[t, 0] + H, M + offs[t, 1]:M + offs[t, 1] + W]
    for t0 in range(0, T, 100):
        raw[t0:t0 + 100] += rs.randint(-30, 30, size=raw[t0:t0 + 100].shape).astype(np.int16)
    tmpl = scene[M:M + H, M:M + W].copy()
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, 'rec.npz')
    np.savez(path, series_raw=raw, name=np.array('synthetic'))

    chunk_bytes = C * H * W * 2
    host = torch.from_numpy(raw[:C].copy()).pin_memory()
    dev = torch.empty((C, H, W), dtype=torch.int16, device='cuda')
    out = torch.empty((C, H, W), dtype=torch.int16, device='cuda')
    dt = torch.from_numpy(tmpl).cuda()
    shifts = torch.zeros((C, 2), dtype=torch.int32, device='cuda')
    bshifts = torch.zeros((C, By, Bx, 2), dtype=torch.int32, device='cuda')
    bscores = torch.empty((C, By, Bx, 2 * D + 1, 2 * D + 1), dtype=torch.int64, device='cuda')
    fine = torch.zeros((C, 2), dtype=torch.int32, device='cuda')
    bfine = torch.zeros((C, By, Bx, 2), dtype=torch.int32, device='cuda')
    frac = torch.tensor([5, 9], dtype=torch.int32, device='cuda')                       # both fractions non-zero
    apart = torch.from_numpy(rs_blocks(C, By, Bx)).cuda()
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn, reps=1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / reps

    def sample(fn, reps=5):
        timed(fn, reps)
        s = [timed(fn, reps) for _ in range(5)]
        return float(np.median(s)), min(s), max(s)

    dev.copy_(host)
    h2d, lo, hi = sample(lambda: dev.copy_(host, non_blocking=True))
    say('(a) H2D copy of one chunk (pinned, %.1f MB)      %8.3f ms  (%.3f - %.3f)  %6.1f GB/s' % (chunk_bytes / 1e6, h2d, lo, hi, chunk_bytes / h2d / 1e6))
    say('(b) per chunk, 5 back to back per sample, median of 5 samples after a warm-up (min - max), and the ratio to the copy:')
    for S in (4, 8, 16):
        nd = 2 * S + 1
        scores = torch.empty((C, nd, nd), dtype=torch.int64, device='cuda')
        madds = C * nd * nd * (H - 2 * S) * (W - 2 * S)
        rows = [('dc_motion_ssd', lambda: L.dc_motion_ssd(dev.data_ptr(), 0, C, dt.data_ptr(), H, W, S, scores.data_ptr(), stream)),
                ('dc_motion_pick', lambda: L.dc_motion_pick(scores.data_ptr(), C, S, shifts.data_ptr(), None, stream)),
                ('dc_motion_apply', lambda: L.dc_motion_apply(dev.data_ptr(), C, shifts.data_ptr(), H, W, 0, out.data_ptr(), stream))]
        total = 0.0
        for name, fn in rows:
            ms, lo, hi = sample(fn)
            total += ms
            ms_apply = ms                                # the last row: dc_motion_apply
            extra = '  %6.2f T multiply-adds/s' % (madds / ms / 1e9) if name == 'dc_motion_ssd' else ''
            say('  S = %2d  %-16s %8.3f ms  (%.3f - %.3f)  / H2D = %5.2f%s' % (S, name, ms, lo, hi, ms / h2d, extra))
        say('  S = %2d  all three       %8.3f ms                     / H2D = %5.2f  (%s)'
            % (S, total, total / h2d, 'hides under the copy' if total < h2d else 'does NOT hide under the copy'))
        bmadds = C * (2 * D + 1) ** 2 * (H - 2 * (S + D)) * (W - 2 * (S + D))
        brows = [('dc_motion_block_ssd', lambda: L.dc_motion_block_ssd(dev.data_ptr(), 0, C, dt.data_ptr(), H, W, S, D, By, Bx, shifts.data_ptr(),
                                                                       bscores.data_ptr(), stream)),
                 ('dc_motion_block_pick', lambda: L.dc_motion_block_pick(bscores.data_ptr(), shifts.data_ptr(), C, By, Bx, S, D,
                                                                         bshifts.data_ptr(), None, stream)),
                 ('dc_motion_warp', lambda: L.dc_motion_warp(dev.data_ptr(), C, bshifts.data_ptr(), By, Bx, H, W, 0, out.data_ptr(), stream))]
        btotal = 0.0
        for name, fn in brows:
            ms, lo, hi = sample(fn)
            btotal += ms
            extra = '  %6.2f T multiply-adds/s' % (bmadds / ms / 1e9) if name == 'dc_motion_block_ssd' else ''
            say('  S = %2d  %-20s %8.3f ms  (%.3f - %.3f)  / H2D = %5.2f%s' % (S, name, ms, lo, hi, ms / h2d, extra))
        say('  S = %2d  piecewise %dx%d, D = %d: these three %8.3f ms, with the rigid ssd and pick %8.3f ms  / H2D = %5.2f'
            % (S, By, Bx, D, btotal, btotal + total - ms_apply, (btotal + total - ms_apply) / h2d))
        ms_warp = ms                                     # the last row: dc_motion_warp
        fine_f, bfine_u, bfine_v = fine.clone(), bfine.clone(), bfine.clone()
        srows = [('dc_motion_refine', lambda: L.dc_motion_refine(scores.data_ptr(), shifts.data_ptr(), C, S, fine.data_ptr(), stream)),
                 ('dc_motion_block_refine', lambda: L.dc_motion_block_refine(bscores.data_ptr(), shifts.data_ptr(), bshifts.data_ptr(), C, By, Bx,
                                                                             S, D, bfine.data_ptr(), stream)),
                 ('dc_motion_apply_sub', lambda: L.dc_motion_apply_sub(dev.data_ptr(), 0, C, fine_f.data_ptr(), H, W, 0, out.data_ptr(), stream)),
                 ('dc_motion_warp_sub, equal', lambda: L.dc_motion_warp_sub(dev.data_ptr(), 0, C, bfine_u.data_ptr(), By, Bx, H, W, 0,
                                                                            out.data_ptr(), stream)),
                 ('dc_motion_warp_sub, apart', lambda: L.dc_motion_warp_sub(dev.data_ptr(), 0, C, bfine_v.data_ptr(), By, Bx, H, W, 0,
                                                                            out.data_ptr(), stream))]
        sub = {}
        for name, fn in srows:
            if name == 'dc_motion_apply_sub':            # the refined shifts are there: move them off the whole pixels
                fine_f.copy_(16 * shifts + frac)
                bfine_u.copy_((16 * shifts + frac)[:, None, None, :].expand(C, By, Bx, 2))
                bfine_v.copy_(bfine_u + apart)
            ms, lo, hi = sample(fn)
            sub[name] = ms
            say('  S = %2d  %-26s %8.3f ms  (%.3f - %.3f)  / H2D = %5.2f' % (S, name, ms, lo, hi, ms / h2d))
        rigid_sub = total - ms_apply + sub['dc_motion_refine'] + sub['dc_motion_apply_sub']
        say('  S = %2d  sub-pixel rigid: ssd, pick, refine, apply_sub %8.3f ms  / H2D = %5.2f  (%s);  apply_sub / apply = %.2f, '
            'warp_sub / warp = %.2f (equal), %.2f (apart)'
            % (S, rigid_sub, rigid_sub / h2d, 'hides under the copy' if rigid_sub < h2d else 'does NOT hide under the copy',
               sub['dc_motion_apply_sub'] / ms_apply, sub['dc_motion_warp_sub, equal'] / ms_warp, sub['dc_motion_warp_sub, apart'] / ms_warp))
        q = (fine.cpu().numpy() - 16 * shifts.cpu().numpy())
        say('  S = %2d  refinements q of the chunk within [-8, 8]: %s (largest |q| %d)' % (S, bool((np.abs(q) <= 8).all()), int(np.abs(q).max())))
        got_b = bshifts.cpu().numpy()
        say('  S = %2d  block shifts of the chunk all equal to the planted rigid shift: %s'
            % (S, bool((got_b == -offs[:C, None, None, :]).all()) if S >= M else 'n/a (S < 5)'))
        got = shifts.cpu().numpy()
        say('  S = %2d  planted shifts of the chunk recovered: %s' % (S, bool((got == -offs[:C]).all()) if S >= M else 'n/a (S < 5)'))

    say('(c) estimate_shifts_device(template given), wall, median of 5 after a warm-up:')
    for S in (4, 8, 16):
        res = []

        def run():
            t = time.perf_counter()
            res[:] = [estimate_shifts_device(path, template=tmpl, max_shift=S, chunk_frames=C)[0]]
            return time.perf_counter() - t
        s = median_of(run)
        say('  S = %2d  %8.3f s  (%.2f GB/s of recording, %.3f ms per chunk)%s'
            % (S, s, T * H * W * 2 / s / 1e9, s * 1e3 / ((T + C - 1) // C),
               '  planted shifts recovered: %s' % bool((res[0] == -offs).all()) if S >= M else ''))

    def run_blocks():
        t = time.perf_counter()
        res[:] = [estimate_shifts_device(path, template=tmpl, max_shift=8, chunk_frames=C, blocks=(By, Bx), max_dev=D)[0]]
        return time.perf_counter() - t
    res = []
    s = median_of(run_blocks)
    say('  S =  8, blocks %dx%d, D = %d  %8.3f s  (%.2f GB/s of recording, %.3f ms per chunk)  block shifts equal the planted rigid ones: %s'
        % (By, Bx, D, s, T * H * W * 2 / s / 1e9, s * 1e3 / ((T + C - 1) // C), bool((res[0] == -offs[:, None, None, :]).all())))

    say('(d) numpy, the same search on %d frames, scaled to a chunk of %d:' % (args.host_frames, C))
    for S in (4, 8, 16):
        def host():
            t = time.perf_counter()
            numpy_scores(raw[:args.host_frames], tmpl, S)
            return (time.perf_counter() - t) * C / args.host_frames
        say('  S = %2d  %8.1f ms per chunk' % (S, median_of(host, n=3, warm=0) * 1e3))
    os.remove(path)
    os.rmdir(tmp)
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
