"""Times of the detrended (segment-pooled) correlations on one GPU (the figures of DESIGN.md section 4j, "Detrended correlations: times").

    python scripts/detrend_speed.py [--hw 512] [--chunk 64] [--rois 300] [--detrend 512] [--out FILE]

One chunk of `--chunk` int16 frames of `--hw` x `--hw`, `--rois` rectangular ROIs of 100 to 400 pixels (footprints with halo 2), a
recording of two segments of `--detrend` frames, i.e. one fold per detrend / chunk chunks.  Timed: the three folds
(dc_series_fold_segment with the pair state, dc_roi_pair_fold_segment, dc_roi_trace_moments + dc_roi_pixel_fold_segment) and the
three pooled finalizes (dc_series_finalize_pooled, dc_roi_pair_corr_pooled, dc_roi_pixel_corr_pooled) -- beside the accumulate
kernels that run on every chunk (dc_series_accumulate + dc_series_accumulate_xy, dc_roi_pair_accumulate, dc_roi_pixel_accumulate)
and the H2D copy of the chunk out of pinned memory.  HIP events on the launch stream around 5 launches back to back; every row is
warmed up once, then ONE run takes 5 rounds in which all rows are timed one after the other (the variants interleaved, so that a
drift of the clock meets all of them alike); the figure is the median of a row's 5 samples (min - max).  Before anything is timed
the readers are fed one whole recording and their one-segment results compared with the undetrended readers' bits.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_rois(n, H, W, rs):
    rois = []
    for _ in range(n):
        h = int(rs.randint(10, 21))
        w = int(rs.randint(10, 21))                      # 100 .. 400 pixels
        y0, x0 = int(rs.randint(0, H - h)), int(rs.randint(0, W - w))
        rois.append(np.array([[y, x] for y in range(y0, y0 + h) for x in range(x0, x0 + w)], np.int64))
    return rois


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--hw', type=int, default=512)
    ap.add_argument('--chunk', type=int, default=64)
    ap.add_argument('--rois', type=int, default=300)
    ap.add_argument('--detrend', type=int, default=512)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    from deep_calcium_amd import RoiFootprints, RoiPairCorr, SeriesSummarizer
    from deep_calcium_amd._lib import lib
    L = lib()
    H = W = args.hw
    C, D = args.chunk, args.detrend
    T = 2 * D
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    nbytes = C * H * W * 2
    rs = np.random.RandomState(0)
    rois = make_rois(args.rois, H, W, rs)
    say('detrended correlations, one chunk of %d x %d x %d int16 (%.1f MB), %d ROIs of %d to %d pixels, L = %d (one fold per %g chunks), %s'
        % (C, H, W, nbytes / 1e6, len(rois), min(len(r) for r in rois), max(len(r) for r in rois), D, D / float(C), torch.cuda.get_device_name(0)))
    stream = torch.cuda.current_stream().cuda_stream
    raw = rs.randint(-32768, 32768, size=(C, H, W)).astype(np.int16)

    # what is timed is right: a short recording of one segment gives the undetrended readers' bits
    short = rs.randint(0, 4096, size=(24, H, W)).astype(np.int16)
    for make in ((lambda **kw: SeriesSummarizer((H, W), 24, np.int16, kinds=('corr',), chunk_frames=8, **kw)),
                 (lambda **kw: RoiPairCorr((H, W), 24, np.int16, rois[:20], chunk_frames=8, **kw)),
                 (lambda **kw: RoiFootprints((H, W), 24, np.int16, rois[:20], chunk_frames=8, **kw))):
        a, b = make(), make(detrend_frames=16)
        for t0 in range(0, 24, 8):
            a.feed(short[t0:t0 + 8])
            b.feed(short[t0:t0 + 8])
        ra, rb = a.result('corr'), b.result('corr')
        ra, rb = (ra, rb) if isinstance(ra, list) else ([ra], [rb])
        assert all(np.array_equal(x.view(np.int32), y.view(np.int32)) for x, y in zip(ra, rb))

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
    fp_ = dev.data_ptr()
    ss = SeriesSummarizer((H, W), T, np.int16, kinds=('std', 'corr'), chunk_frames=C, detrend_frames=D)
    pc = RoiPairCorr((H, W), T, np.int16, rois, chunk_frames=C, detrend_frames=D)
    fo = RoiFootprints((H, W), T, np.int16, rois, halo=2, chunk_frames=C, detrend_frames=D)
    fo._ext.sums.zero_()                                 # dc_roi_trace_moments reads the whole segment's columns
    for reader in (ss, pc, fo):                          # the first chunk through the readers' own path: every state is initialised
        reader.feed(dev)
    mult = D
    img = torch.empty((3, H * W), dtype=torch.float32, device='cuda')
    pcorr = torch.empty((pc.n_state,), dtype=torch.float32, device='cuda')
    fcorr = torch.empty((fo.n_entries,), dtype=torch.float32, device='cuda')
    say('state: series %d pixels; pairs %d ROI pixels, %d matrix entries in %d tiles; footprints %d entries in %d rows'
        % (H * W, pc.n_pixels, pc.n_state, pc.n_tiles, fo.n_entries, fo._rows))

    def series_acc():
        L.dc_series_accumulate(fp_, 0, C, C, D, None, None, ss.sum.data_ptr(), ss.sumsq.data_ptr(), ss.vmax.data_ptr(), H, W, stream)
        L.dc_series_accumulate_xy(fp_, 0, C, C, ss.xy.data_ptr(), H, W, stream)

    def series_fold():
        L.dc_series_fold_segment(ss.sum.data_ptr(), ss.sumsq.data_ptr(), ss.xy.data_ptr(), ss.vmax.data_ptr(), D, mult, ss._pvar.data_ptr(),
                                 ss._pcov.data_ptr(), ss._sum_total.data_ptr(), ss._vmax_total.data_ptr(), H, W, stream)

    def series_fin():
        L.dc_series_finalize_pooled(ss._pvar.data_ptr(), ss._pcov.data_ptr(), ss._sum_total.data_ptr(), img[0].data_ptr(), img[1].data_ptr(),
                                    img[2].data_ptr(), H, W, D * D, T, stream)

    def pair_fold():
        L.dc_roi_pair_fold_segment(pc._a.data_ptr(), pc._g.data_ptr(), pc._roi_off.data_ptr(), pc._goff.data_ptr(), pc._tiles.data_ptr(),
                                   pc.n_tiles, pc.n_rois, pc.n_pixels, pc.n_state, D, mult, pc._pooled.data_ptr(), stream)

    def pair_fin():
        L.dc_roi_pair_corr_pooled(pc._pooled.data_ptr(), pc._roi_off.data_ptr(), pc._goff.data_ptr(), pc.n_rois, pc.n_pixels, pc.n_state,
                                  pcorr.data_ptr(), stream)

    def pixel_fold():
        L.dc_roi_trace_moments(fo._ext.sums.data_ptr(), T, fo.n_rois, D, fo._rmom.data_ptr(), stream)
        L.dc_roi_pixel_fold_segment(fo._mom.data_ptr(), fo.n_entries, fo._row_off.data_ptr(), fo._row_roi.data_ptr(), fo._rows, fo.n_rois,
                                    fo._rmom.data_ptr(), D, mult, fo._pxx.data_ptr(), fo._pxs.data_ptr(), fo._pss.data_ptr(), H, W, stream)

    def pixel_fin():
        L.dc_roi_pixel_corr_pooled(fo._pxx.data_ptr(), fo._pxs.data_ptr(), fo._pss.data_ptr(), fo.n_entries, fo._row_off.data_ptr(),
                                   fo._row_roi.data_ptr(), fo._rows, fo.n_rois, fo._flags.data_ptr(), fcorr.data_ptr(), stream)

    rows = [('h2d', 'H2D copy of the chunk (pinned)', lambda: dev.copy_(host, non_blocking=True)),
            ('s_acc', 'dc_series_accumulate + _xy', series_acc),
            ('p_acc', 'dc_roi_pair_accumulate', lambda: pc._accumulate_frames(fp_, C, stream)),
            ('x_acc', 'dc_roi_pixel_accumulate', lambda: fo._accumulate_frames(fp_, C, 0, stream)),
            ('s_fold', 'dc_series_fold_segment', series_fold),
            ('p_fold', 'dc_roi_pair_fold_segment', pair_fold),
            ('x_fold', 'dc_roi_trace_moments + dc_roi_pixel_fold_segment', pixel_fold),
            ('s_fin', 'dc_series_finalize_pooled', series_fin),
            ('p_fin', 'dc_roi_pair_corr_pooled', pair_fin),
            ('x_fin', 'dc_roi_pixel_corr_pooled', pixel_fin)]
    for _, _, fn in rows:                                # warm-up
        timed(fn, 1)
    samples = dict((key, []) for key, _, _ in rows)
    for _ in range(5):                                   # one run, the variants interleaved
        for key, _, fn in rows:
            samples[key].append(timed(fn))
    med = dict((k, (float(np.median(v)), min(v), max(v))) for k, v in samples.items())
    h2d = med['h2d'][0]
    per = D / float(C)
    say('per call, 5 launches back to back per sample, median of 5 interleaved samples after a warm-up (min - max); a fold runs once per')
    say('%g chunks, a finalize once per recording:' % per)
    for key, label, _ in rows:
        ms, lo, hi = med[key]
        extra = '  per chunk %.4f ms = %.3f of the copy' % (ms / per, ms / per / h2d) if key.endswith('_fold') else ''
        say('  %-50s %8.3f ms  (%.3f - %.3f)%s' % (label, ms, lo, hi, extra))
    folds = sum(med[k][0] for k in ('s_fold', 'p_fold', 'x_fold')) / per
    say('the three folds together, amortised: %.4f ms per chunk, which %s under the copy of %.3f ms'
        % (folds, 'stays' if folds < h2d else 'does NOT stay', h2d))
    if args.out:
        with open(args.out, 'w') as fp:
            fp.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
