"""Times of the ROI footprint-map kernels on one GPU (the figures of DESIGN.md section 4h).

    python scripts/roi_footprint_speed.py [--frames 64] [--hw 512] [--rois 300] [--out FILE]

One chunk of `--frames` synthetic int16 frames of `--hw` x `--hw`; the ROIs are `--rois` discs of 100-400 pixels at random
centres (scripts/roi_trace_speed.py's, without its whole-image ROI).  Per halo in (0, 2), timed in the same run with HIP events on
the launch stream around 20 launches back to back, median of 5 such samples after a warm-up (min - max):
 (a) dc_roi_pixel_accumulate on the chunk, over the supports cut into CSR rows as RoiFootprints does;
 (b) the two yardsticks: dc_roi_trace_accumulate on the same chunk and ROIs (the same gather without the products), and the
     chunk's H2D copy out of pinned memory -- the pass stays hidden while (a) + trace < copy;
 (c) dc_roi_trace_moments and dc_roi_pixel_corr, which run once per recording (timed over the chunk's frames as the recording).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.roi_trace_speed import make_rois          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--hw', type=int, default=512)
    ap.add_argument('--rois', type=int, default=300)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from deep_calcium_amd import roi_support, rois_to_csr
    from deep_calcium_amd._lib import lib
    L = lib()
    C, H, W = args.frames, args.hw, args.hw
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    chunk_bytes = C * H * W * 2
    say('ROI footprint maps, one chunk of %d x %d x %d int16 (%.1f MB), %s' % (C, H, W, chunk_bytes / 1e6, torch.cuda.get_device_name(0)))
    rs = np.random.RandomState(0)
    raw = (rs.randint(100, 1200, size=(1, H, W)) + rs.randint(-90, 600, size=(C, H, W))).astype(np.int16)
    rois = make_rois(H, W, args.rois, rs)[:-1]
    areas, own_off, own_pix, own_roi = rois_to_csr(rois, (H, W))
    R = len(areas)
    say('%d ROIs, %d pixels (median area %d, largest %d)' % (R, int(areas.sum()), int(np.median(areas)), int(areas.max())))
    host = torch.from_numpy(raw).pin_memory()
    dev = torch.empty((C, H, W), dtype=torch.int16, device='cuda')
    dev.copy_(host)
    d_own = [torch.from_numpy(a).cuda() for a in (own_off, own_pix, own_roi)]
    sums = torch.zeros((R, C), dtype=torch.int64, device='cuda')
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

    def sample(name, fn, bytes_moved=None):
        timed(fn, 20)
        samples = [timed(fn, 20) for _ in range(5)]
        ms = float(np.median(samples))
        rate = '' if bytes_moved is None else '  %8.1f GB/s' % (bytes_moved / ms / 1e6)
        say('  %-52s %8.4f ms  (%.4f - %.4f)%s' % (name, ms, min(samples), max(samples), rate))
        return ms

    def trace():
        L.dc_roi_trace_accumulate(dev.data_ptr(), 0, C, 0, d_own[0].data_ptr(), d_own[1].data_ptr(), d_own[2].data_ptr(), len(own_roi), R,
                                  sums.data_ptr(), C, H, W, stream)

    say('per chunk, 20 back to back per sample, median of 5 samples after a warm-up (min - max):')
    h2d = sample('H2D copy of the chunk (pinned)', lambda: dev.copy_(host, non_blocking=True), chunk_bytes)
    tr = sample('dc_roi_trace_accumulate (%d rows)' % len(own_roi), trace, 2.0 * C * int(areas.sum()))
    for halo in (0, 2):
        coords, inside = roi_support(rois, (H, W), halo)
        counts, row_off, row_pix, row_roi = rois_to_csr(coords, (H, W))
        N, S = int(counts.sum()), len(row_roi)
        d_off, d_pix, d_roi = (torch.from_numpy(a).cuda() for a in (row_off, row_pix, row_roi))
        flags = torch.from_numpy(np.concatenate(inside).astype(np.int32)).cuda()
        mom = torch.zeros((4, N), dtype=torch.int64, device='cuda')
        rmom = torch.zeros((3, R), dtype=torch.int64, device='cuda')
        corr = torch.zeros((N,), dtype=torch.float32, device='cuda')
        say('halo %d: %d support entries in %d CSR rows (%.2f entries per ROI pixel)' % (halo, N, S, N / float(areas.sum())))
        px = sample('dc_roi_pixel_accumulate',
                    lambda: L.dc_roi_pixel_accumulate(dev.data_ptr(), 0, C, 0, d_off.data_ptr(), d_pix.data_ptr(), d_roi.data_ptr(), S, R,
                                                      sums.data_ptr(), C, mom.data_ptr(), N, H, W, stream), 2.0 * C * N)
        say('    / dc_roi_trace_accumulate = %.2f;  per gathered pixel %.2f of the trace kernel;  (pixel + trace) / H2D = %.3f  (%s)'
            % (px / tr, (px / N) / (tr / float(areas.sum())), (px + tr) / h2d,
               'hidden under the copy' if px + tr < h2d else 'NOT hidden: %.3f ms over the copy' % (px + tr - h2d)))
        sample('dc_roi_trace_moments (T = %d)' % C, lambda: L.dc_roi_trace_moments(sums.data_ptr(), C, R, C, rmom.data_ptr(), stream))
        sample('dc_roi_pixel_corr',
               lambda: L.dc_roi_pixel_corr(mom.data_ptr(), N, d_off.data_ptr(), d_roi.data_ptr(), S, R, flags.data_ptr(), rmom.data_ptr(), C,
                                           corr.data_ptr(), stream))
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
