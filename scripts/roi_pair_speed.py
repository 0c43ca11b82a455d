"""Times of the ROI pixel-pair correlation kernels on one GPU (the figures of DESIGN.md section 4i).

    python scripts/roi_pair_speed.py [--frames 64] [--hw 512] [--rois 300] [--out FILE]

One chunk of `--frames` synthetic int16 frames of `--hw` x `--hw`; the ROIs are `--rois` discs of 100-400 pixels at random
centres (scripts/roi_trace_speed.py's, without its whole-image ROI).  Timed in ONE run with HIP events on the launch stream, the
variants interleaved: in every round each variant in turn runs 20 launches back to back between two events; the figure is the
median over 7 rounds after a warm-up round (min - max):
 (a) dc_roi_pair_accumulate on the chunk, over the tile list RoiPairCorr builds;
 (b) the yardsticks: dc_roi_trace_accumulate and dc_roi_pixel_accumulate (halo 0) on the same chunk and ROIs, and the chunk's
     H2D copy out of pinned memory -- the pass stays hidden while (a) + trace < copy;
 (c) dc_roi_pair_corr, which runs once per recording (timed once, after a warm-up, over the chunk's frames as the recording).
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
    from deep_calcium_amd.roi_pairs import pair_layout
    from deep_calcium_amd.traces import _roi_pixels
    L = lib()
    C, H, W = args.frames, args.hw, args.hw
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    chunk_bytes = C * H * W * 2
    say('ROI pixel-pair correlation, one chunk of %d x %d x %d int16 (%.1f MB), %s' % (C, H, W, chunk_bytes / 1e6, torch.cuda.get_device_name(0)))
    rs = np.random.RandomState(0)
    raw = (rs.randint(100, 1200, size=(1, H, W)) + rs.randint(-90, 600, size=(C, H, W))).astype(np.int16)
    rois = make_rois(H, W, args.rois, rs)[:-1]
    areas, own_off, own_pix, own_roi = rois_to_csr(rois, (H, W))
    R = len(areas)
    pixels = _roi_pixels(rois, (H, W))
    roi_off, goff, tiles, G = pair_layout([len(p) for p in pixels])
    P, ntiles = int(roi_off[-1]), len(tiles)
    pairs = int(sum(int(k) * (int(k) + 1) // 2 for k in areas))
    say('%d ROIs, %d pixels (median area %d, largest %d); %d pairs i <= j in %d tiles, state %d words (%.1f MB)' % (
        R, P, int(np.median(areas)), int(areas.max()), pairs, ntiles, G, 8 * G / 1e6))
    host = torch.from_numpy(raw).pin_memory()
    dev = torch.empty((C, H, W), dtype=torch.int16, device='cuda')
    dev.copy_(host)
    d_own = [torch.from_numpy(a).cuda() for a in (own_off, own_pix, own_roi)]
    sums = torch.zeros((R, C), dtype=torch.int64, device='cuda')
    coords, inside = roi_support(rois, (H, W), 0)
    counts, row_off, row_pix, row_roi = rois_to_csr(coords, (H, W))
    N, S = int(counts.sum()), len(row_roi)
    d_sup = [torch.from_numpy(a).cuda() for a in (row_off, row_pix, row_roi)]
    mom = torch.zeros((4, N), dtype=torch.int64, device='cuda')
    d_off, d_goff, d_tiles = torch.from_numpy(roi_off).cuda(), torch.from_numpy(goff).cuda(), torch.from_numpy(np.ascontiguousarray(tiles)).cuda()
    d_pix = torch.from_numpy(np.concatenate(pixels).astype(np.int32)).cuda()
    a = torch.zeros((P,), dtype=torch.int64, device='cuda')
    g = torch.zeros((G,), dtype=torch.int64, device='cuda')
    corr = torch.zeros((G,), dtype=torch.float32, device='cuda')
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn, reps=1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    variants = [
        ('H2D copy of the chunk (pinned)', lambda: dev.copy_(host, non_blocking=True), chunk_bytes),
        ('dc_roi_trace_accumulate (%d rows)' % len(own_roi),
         lambda: L.dc_roi_trace_accumulate(dev.data_ptr(), 0, C, 0, d_own[0].data_ptr(), d_own[1].data_ptr(), d_own[2].data_ptr(), len(own_roi), R,
                                           sums.data_ptr(), C, H, W, stream), 2.0 * C * P),
        ('dc_roi_pixel_accumulate (halo 0, %d rows)' % S,
         lambda: L.dc_roi_pixel_accumulate(dev.data_ptr(), 0, C, 0, d_sup[0].data_ptr(), d_sup[1].data_ptr(), d_sup[2].data_ptr(), S, R,
                                           sums.data_ptr(), C, mom.data_ptr(), N, H, W, stream), 2.0 * C * N),
        ('dc_roi_pair_accumulate (%d tiles)' % ntiles,
         lambda: L.dc_roi_pair_accumulate(dev.data_ptr(), 0, C, d_off.data_ptr(), d_pix.data_ptr(), d_goff.data_ptr(), d_tiles.data_ptr(), ntiles,
                                          R, a.data_ptr(), g.data_ptr(), P, G, H, W, stream), None),
    ]
    rounds = [[timed(fn, 20) for _, fn, _ in variants] for _ in range(8)][1:]       # the first round is the warm-up
    say('per chunk, 20 back to back per sample, the variants in turn, median of 7 rounds after a warm-up round (min - max):')
    ms = []
    for n, (name, _, moved) in enumerate(variants):
        samples = [r[n] for r in rounds]
        ms.append(float(np.median(samples)))
        rate = '' if moved is None else '  %8.1f GB/s' % (moved / ms[-1] / 1e6)
        say('  %-52s %8.4f ms  (%.4f - %.4f)%s' % (name, ms[-1], min(samples), max(samples), rate))
    h2d, tr, px, pr = ms
    say('    pair: %.1f G multiply-adds/s over the pairs i <= j (%.2f G/s over the tiles\' %d x %d);  / dc_roi_pixel_accumulate = %.1f'
        % (pairs * C / pr / 1e6, ntiles * 64 * 64 * C / pr / 1e6, 64, 64, pr / px))
    say('    (pair + trace) / H2D = %.3f  (%s)' % ((pr + tr) / h2d, 'hidden under the copy' if pr + tr < h2d
                                                   else 'NOT hidden: %.3f ms over the copy' % (pr + tr - h2d)))

    def pair_corr():
        L.dc_roi_pair_corr(a.data_ptr(), g.data_ptr(), d_off.data_ptr(), d_goff.data_ptr(), R, P, G, C, corr.data_ptr(), stream)
    timed(pair_corr)
    say('once per recording:')
    say('  %-52s %8.4f ms  (one launch, %d values)' % ('dc_roi_pair_corr (T = %d)' % C, timed(pair_corr), G))
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
