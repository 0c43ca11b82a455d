#!/usr/bin/env python
"""Neurofinder training, evaluation and prediction with the HIP UNet2DS path: the reference's example
(/root/reference/examples/neurons/unet2ds_nf.py) with the same three actions, arguments, seeds and call sequence, on
`deep_calcium_amd.UNet2DSummary`, plus `traces`: predict the neurons' mask, then extract one fluorescence trace per neuron from
`series/raw` on the GPU and write the file the reference's spikes model reads (models/spikes/unet_1d_segmentation.py:182-187).

    python examples/neurons/unet2ds_nf.py evaluate neurofinder.00.00 --model unet2ds_model.hdf5
    python examples/neurons/unet2ds_nf.py train all_train [-m model.hdf5] [-c checkpoints_dir]
    python examples/neurons/unet2ds_nf.py predict all_test --model unet2ds_model.hdf5
    python examples/neurons/unet2ds_nf.py traces neurofinder.00.00 --model unet2ds_model.hdf5 [--kind mean|zscore|sum] [--register [S] [--blocks ByxBx [--max-dev D]] [--coarse C] [--subpixel]] [--bidi [P]] [--dff WINDOW [--percentile Q] [--neuropil INNER,OUTER,WEIGHT] [--deconvolve auto|each|TAU [--fps F] [--spike-rise TAU_RISE] [--spike-k K | --spike-constrain s_min|lam] [--spike-baseline fit|VALUE]]] [--refine THR [--halo N]] [--split [GAP] [--min-area N]] [--bin-frames B] [--detrend L] [--merge [THR] [--merge-dist D]] [--weighted [FLOOR] [--overlap keep|exclude|demix]]

`--model` takes the reference's own files: the released Keras `unet2ds_model.hdf5`
(unet_2d_summary.py:28), any Keras ModelCheckpoint file, or a checkpoint written by this build.  With the released
weights and the Neurofinder data in place, `evaluate neurofinder.00.00` is the one command whose output the reference's
README quotes (prec=0.976, reca=1.000, comb=0.988 with TTA; 0.919 / 1.000 / 0.958 without: /root/reference/README.md:30-37)
-- neither is available offline, so that comparison cannot be run inside the build container.

Datasets: names (`neurofinder.00.00`, comma lists, `all`, `all_train`, `all_test`) go through
`deep_calcium_amd.nf_datasets.nf_load_hdf5` (the reference's datasets/nf.py:37-150): <datasets_dir>/neurons_nf/<name>/
dataset.hdf5 is built from the unpacked challenge directory (images/*.tiff + regions/regions.json; the zip is fetched
first when the machine has network access); paths to existing .hdf5 / .npz dataset files are taken as they are.
Multi-GPU training: launch with `python -m torch.distributed.run --nproc-per-node N examples/neurons/unet2ds_nf.py train ...`.
"""
from time import time
import argparse
import logging
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))

from deep_calcium_amd import (UNet2DSummary, parallel, extract_traces_device, write_traces_dataset,      # noqa: E402
                              estimate_shifts_device, estimate_bidi_device, summarize_series_device, valid_rectangle, dff_traces_device, roi_footprints_device, refine_rois,
                              split_rois_device, detrend_plan, merge_rois_device, make_template, frame_quality_device, flag_frames,
                              footprint_weights, exclude_overlap, weighted_traces_device, TraceDeconvolver, ar1_gamma, trace_noise,
                              TraceDynamics, pick_gamma, ar1_tau, TraceDynamicsAR2, pick_roots)
from deep_calcium_amd.weighted import shared_pixels            # noqa: E402
from deep_calcium_amd.deconv import ar2_coefficients, ar2_peak   # noqa: E402
from deep_calcium_amd.nf_metrics import nf_submit                # noqa: E402
from deep_calcium_amd.nf_datasets import nf_load_hdf5, default_dirs      # noqa: E402

DATASETS_DIR, CHECKPOINTS_DIR = default_dirs()                   # ~/.deep-calcium/deep-calcium.json or the defaults
CHECKPOINTS_DIR = '%s/neurons_unet2ds_nf' % CHECKPOINTS_DIR      # reference :16

np.random.seed(865)                 # examples/neurons/unet2ds_nf.py:18: the batch generator's stream
# :19 tf.set_random_seed(7535) seeds TF's dropout / initialisers; here 7535 is the default `seed` of unet_hip's engine
# (initial weights + the counter-hash dropout stream) -- TF's Philox stream itself is not reproducible outside TF
logging.basicConfig(level=logging.INFO)


def nf_find_hdf5(names, datasets_dir=os.path.join(DATASETS_DIR, 'neurons_nf')):
    """names -> dataset files.  Explicit paths of existing dataset .hdf5 / .npz files pass through; Neurofinder names go
    to nf_load_hdf5 (the reference's datasets/nf.py:37-150), which builds `<datasets_dir>/<name>/dataset.hdf5` from the
    unpacked challenge directory (images/*.tiff, regions/regions.json), fetching the zip first if it can."""
    if isinstance(names, str) and names.lower() not in ('all', 'all_train', 'all_test'):
        names = names.split(',')
    if not isinstance(names, str) and all(os.path.isfile(n) for n in names):
        return list(names)
    try:
        return nf_load_hdf5(names, datasets_dir=datasets_dir)
    except (IOError, KeyError) as e:
        raise SystemExit('dataset %r: %s' % (names, e))


def training(dataset_name, model_path, checkpoints_dir, nb_steps=100, nb_epochs=10):
    """Train on neurofinder datasets (reference :23-44, same hyper-parameters; --nb_steps / --nb_epochs are additions
    for short runs, the defaults are the reference's 100 x 10)."""
    parallel.init_from_env()                       # no-op unless launched with torch.distributed.run
    dspaths = nf_find_hdf5(dataset_name)           # every rank calls it: rank 0 builds missing dataset files, the others wait inside
    model = UNet2DSummary(cpdir=checkpoints_dir)
    return model.fit(
        dspaths,
        model_path=model_path,
        shape_trn=(128, 128),
        shape_val=(512, 512),
        batch_size_trn=20,
        nb_steps_trn=nb_steps,
        nb_epochs=nb_epochs,
        keras_callbacks=[],
        prop_trn=0.75,
        prop_val=0.25,
    )


def evaluation(dataset_name, model_path, checkpoints_dir):
    """Evaluate datasets -- once with test-time augmentation and once without (reference :47-64)."""
    logger = logging.getLogger('evaluation')
    ds_trn = nf_find_hdf5(dataset_name)
    model = UNet2DSummary(cpdir=checkpoints_dir)
    for aug in [True, False]:
        logger.info('Evaluation with%s.' % (' TTA' if aug else 'out TTA'))
        model.predict(ds_trn, model_path=model_path, window_shape=(512, 512), save=True, print_scores=True, augmentation=aug)


def prediction(dataset_name, model_path, checkpoints_dir):
    """Predictions + Neurofinder submission files with and without test-time augmentation (reference :67-96)."""
    logger = logging.getLogger('prediction')
    ds_tst = nf_find_hdf5(dataset_name)
    model = UNet2DSummary(cpdir=checkpoints_dir)
    tic = int(time())
    for aug in [True, False]:
        logger.info('Prediction with%s.' % (' TTA' if aug else 'out TTA'))
        Mp, names = model.predict(ds_tst, model_path=model_path, window_shape=(512, 512), save=False, augmentation=aug)
        Mp = [m.round() for m in Mp]
        nf_submit(Mp, names, '%s/submission_%d%s.json' % (model.cpdir, tic, ('_TTA' if aug else '')))
        nf_submit(Mp, names, '%s/submission_latest%s.json' % (model.cpdir, ('_TTA' if aug else '')))


def _blocks_arg(text):
    """'4x4' -> (4, 4)."""
    try:
        by, bx = (int(v) for v in text.lower().split('x'))
    except ValueError:
        raise argparse.ArgumentTypeError('expected ByxBx, e.g. 4x4, not %r' % text)
    return by, bx


def _neuropil_arg(text):
    try:
        inner, outer, weight = text.split(',')
        return int(inner), int(outer), float(weight)
    except ValueError:
        raise argparse.ArgumentTypeError('expected INNER,OUTER,WEIGHT such as 2,12,0.7, not %r' % text)


def _deconvolve_arg(text):
    """'auto' | 'each' | a decay time in seconds."""
    if text in ('auto', 'each'):
        return text
    try:
        return float(text)
    except ValueError:
        raise argparse.ArgumentTypeError('expected auto, each or the decay time TAU in seconds, not %r' % text)


def _rise_arg(text):
    """'auto' | a rise time in seconds."""
    if text == 'auto':
        return text
    try:
        return float(text)
    except ValueError:
        raise argparse.ArgumentTypeError('expected auto or the rise time TAU_RISE in seconds, not %r' % text)


def _baseline_arg(text):
    """'fit' | a constant."""
    if text == 'fit':
        return text
    try:
        return float(text)
    except ValueError:
        raise argparse.ArgumentTypeError('expected fit or a constant VALUE, not %r' % text)


def _n_frames(dspath):
    from deep_calcium_amd.series import _open_series
    frames, close = _open_series(dspath, 'series/raw')
    try:
        return int(frames.shape[0])
    finally:
        frames = None
        close()


def traces(dataset_name, model_path, checkpoints_dir, kind='mean', register=None, blocks=None, max_dev=3, subpixel=False, dff=None,
           percentile=8, neuropil=None, refine=None, halo=2, coarse=None, split=None, min_area=8, bidi=None,
           bin_frames=None, detrend=None, merge=None, merge_dist=2, drop_artefacts=None, weighted=None, overlap='keep', deconvolve=None,
           fps=None, spike_k=3.0, spike_constrain=None, spike_baseline=None, spike_rise=None):
    """Mask -> traces: predict each dataset's neurons (with TTA), take the 8-connected regions of the rounded mask as ROIs and
    write `<checkpoints_dir>/<name>_traces.hdf5` with one trace per region over `series/raw` (no reference counterpart: its spikes
    model starts from such a file).  register=S: the frames of `series/raw` are first registered on the GPU (rigid, whole pixels,
    within +-S); the summary the network segments is then the mean of the registered raw frames instead of the stored
    `series/mean`, and the traces are summed over the registered frames.  blocks=(By, Bx) with register: piecewise-rigid -- every
    block of the frame gets the rigid shift plus a residual within +-max_dev, and the frames are warped by the blended field.
    subpixel with register: every shift is refined to a sixteenth of a pixel and the frames are interpolated bilinearly.
    coarse=C (2, 4 or 8) with register: the wide search -- a coarse shift on frames binned C x C, then the whole-pixel shifts within
    +-C of it --, which lets S reach 16 C (`--register 48 --coarse 4`); rigid only.
    dff=WINDOW: instead of `kind`, the traces are dF/F against a rolling-percentile baseline over WINDOW frames (odd; `percentile`,
    default 8), after subtracting neuropil=(inner, outer, weight) times the trace of a ring around every ROI when given.
    refine=THR: a first pass over the recording computes every ROI's footprint map (the correlation of each pixel of the ROI and of
    a `halo` around it with the ROI's trace); every ROI is cut down (or grown) to the largest connected set of pixels with
    correlation >= THR, ROIs with none are dropped, and the traces are those of the refined ROIs (a second pass).
    split=GAP: one more pass over the recording (after the refinement, where both are given) computes the correlation of every
    pixel of an ROI with every other one; an ROI whose pixels fall into two groups, each of at least `min_area` pixels and more
    correlated within than across by GAP (deep_calcium_amd.split_rois), becomes two ROIs with a trace each.
    bidi=P (with or without register): the scan-phase offset of the odd lines is searched within +-P over the first 200 frames of
    `series/raw` first, and every later step -- the registration and its template, the summary the network segments, the
    footprints, the split, the traces -- reads frames whose odd lines have been moved back by it.
    bin_frames=B (with refine or split): those two passes correlate the rounded means of B consecutive corrected frames
    (deep_calcium_amd.TemporalBinner: the pixel noise falls by sqrt(B), a transient of many frames survives; the trailing T % B
    frames are dropped).  The traces that are written are always those of every frame.  Keep T // B well above 100.
    detrend=L (with refine or split): those two passes correlate WITHIN segments of L frames (binned frames with bin_frames) and pool
    the segments (`detrend_frames=` of the readers): bleaching and drift that are common to all pixels no longer push every
    correlation towards 1.  Piecewise-constant detrending: a trend inside a segment stays, and short segments also remove real slow
    covariance.  The traces that are written are not detrended (--dff is for that).
    merge=THR: one more pass over the recording (after the refinement and the split, where given) sums every ROI's trace; ROIs whose
    pixels lie within `merge_dist` pixels of each other (Chebyshev; 2: one blank pixel between) and whose traces correlate at THR or
    above become one ROI (deep_calcium_amd.merge_rois: single linkage, one round) -- one cell that the mask delivers in fragments is
    counted once.  detrend applies to this correlation too, and a recording that bleaches needs it: a common decay pushes every
    trace pair towards 1 and merges distinct neighbours.
    drop_artefacts=K: one more pass over the recording (after bidi and register, with their corrections) scores every frame -- its
    mean and its correlation with the template over the rectangle every corrected frame covers (deep_calcium_amd.FrameQuality); the
    template is the registration's, or without one the rounded mean of the first 200 frames.  Frames whose mean lies more than K
    scaled median absolute deviations from the median, or whose correlation lies that far BELOW it (deep_calcium_amd.flag_frames),
    are artefact frames -- a stimulation flash, a gated PMT, a z-jump: the summary the network segments, the refinement, the split
    and the merge leave them out (`keep=`).  The traces that are written keep every frame.
    weighted=FLOOR: after the refinement, the split and the merge, one more footprint pass over the final ROIs; every pixel gets the
    weight floor(256 max(corr, 0) + 0.5) of its correlation with its ROI's trace (deep_calcium_amd.footprint_weights; pixels with
    corr < FLOOR or weight 0 are dropped, ROIs left empty too) and the traces are the weighted ones (kind, or dF/F with the weight
    sum where the area stood).  overlap (with weighted): 'keep' -- a pixel two ROIs share counts for both --, 'exclude' -- shared
    pixels are dropped from all --, 'demix' -- the least-squares coefficients of the footprints (deep_calcium_amd.demix_traces,
    float64; z-scored with --kind zscore); not together with dff, whose kernels take integers.
    deconvolve=TAU (with dff and fps=F): spikes without a trained model -- the dF/F traces are deconvolved on the GPU with the AR(1)
    decay g = exp(-1 / (TAU F)) (TAU: the indicator's decay time in seconds, F: frames a second) and the smallest spike
    spike_k * sigma_hat of every trace (deep_calcium_amd.TraceDeconvolver, trace_noise); the file gets the float64 datasets
    `calcium` and `deconvolved` (the spikes; an event is a value > 0) beside `traces`.  deconvolve='auto' or 'each' (fps optional):
    the decay is estimated from the dF/F itself, per trace, from its autocovariance (deep_calcium_amd.TraceDynamics, pick_gamma);
    'auto' deconvolves every trace with the pooled median, 'each' with the trace's own estimate.  spike_constrain='s_min' or 'lam':
    no spike_k -- that parameter is searched per trace on the GPU until the residual equals the noise (TraceDeconvolver(constrain=));
    s_min is the one for events, lam gives a denoised calcium.  spike_baseline='fit': one constant per trace is fitted inside the
    deconvolution, on the GPU (TraceDeconvolver(baseline='fit')): dF/F over a low percentile sits about one sigma_hat above zero
    when the cell is quiet, which costs spurious events; recommended together with spike_constrain, since with a spike_k that is
    too high the missed events lift the fitted baseline.  spike_baseline=VALUE (not with spike_constrain): that constant is taken
    off every trace.  spike_rise=TAU_RISE (with deconvolve=TAU, not auto or each, and not with spike_baseline='fit'): the indicator's
    rise time in seconds; the model is then AR(2) with the roots exp(-1 / (TAU F)) and exp(-1 / (TAU_RISE F))
    (TraceDeconvolver(rise=)), which keeps an event whose fluorescence takes several frames to peak from being reported as a run
    of spikes.  spike_rise='auto' (with deconvolve='auto'): both roots are estimated from the dF/F (deep_calcium_amd.TraceDynamicsAR2,
    pick_roots: the coefficients per trace, the medians of decay and rise over the traces that give two real roots in (0, 1)) and
    the pooled pair serves all traces."""
    logger = logging.getLogger('traces')
    if blocks is not None and register is None:
        raise ValueError('--blocks needs --register')
    if subpixel and register is None:
        raise ValueError('--subpixel needs --register')
    if coarse is not None and register is None:
        raise ValueError('--coarse needs --register')
    if coarse is not None and blocks is not None:
        raise ValueError('--coarse together with --blocks is not built: the piecewise-rigid mode needs --register <= 16')
    if bidi is not None and not 0 <= bidi <= 16:
        raise ValueError('--bidi searches within +-P pixels, P in [0, 16], not %d' % bidi)
    if dff is None and neuropil is not None:
        raise ValueError('--neuropil needs --dff')
    if deconvolve is not None and dff is None:
        raise ValueError('--deconvolve needs --dff: the deconvolution has no baseline term')
    estimated = isinstance(deconvolve, str)
    if estimated and deconvolve not in ('auto', 'each'):
        raise ValueError('--deconvolve takes auto, each or the decay time TAU in seconds, not %r' % (deconvolve,))
    if deconvolve is not None and not estimated and fps is None:
        raise ValueError('--deconvolve needs --fps: the decay per frame is exp(-1 / (TAU * fps))')
    if spike_constrain is not None and deconvolve is None:
        raise ValueError('--spike-constrain needs --deconvolve')
    if spike_constrain not in (None, 's_min', 'lam'):
        raise ValueError('--spike-constrain takes s_min or lam, not %r' % (spike_constrain,))
    if spike_baseline is not None and deconvolve is None:
        raise ValueError('--spike-baseline needs --deconvolve')
    if spike_baseline is not None and spike_baseline != 'fit':
        if isinstance(spike_baseline, str) or not np.isfinite(spike_baseline):
            raise ValueError('--spike-baseline takes fit or a finite constant, not %r' % (spike_baseline,))
        if spike_constrain is not None:
            raise ValueError('--spike-baseline VALUE cannot go with --spike-constrain: the search fits the baseline (fit) or has none')
    base_kw = {} if spike_baseline is None else dict(baseline=spike_baseline)
    if deconvolve is not None and not spike_k >= 0:
        raise ValueError('--spike-k is the smallest spike in units of the trace noise, K >= 0, not %r' % (spike_k,))
    g = None if deconvolve is None or estimated else ar1_gamma(deconvolve, fps)
    rise = None
    if isinstance(spike_rise, str):
        if spike_rise != 'auto':
            raise ValueError('--spike-rise takes auto or the rise time TAU_RISE in seconds, not %r' % (spike_rise,))
        if deconvolve != 'auto':
            raise ValueError('--spike-rise auto estimates both roots, pooled over the traces: it needs --deconvolve auto')
        if spike_baseline == 'fit':
            raise ValueError('--spike-baseline fit is not built for AR(2) (--spike-rise)')
    elif spike_rise is not None:
        if g is None:
            raise ValueError('--spike-rise needs --deconvolve TAU: estimating the decay (auto, each) is not built for AR(2)')
        if spike_baseline == 'fit':
            raise ValueError('--spike-baseline fit is not built for AR(2) (--spike-rise)')
        rise = ar1_gamma(spike_rise, fps)
        if not rise < g:
            raise ValueError('--spike-rise must be shorter than the decay time: TAU_RISE = %r against TAU = %r' % (spike_rise, deconvolve))
        base_kw = dict(base_kw, rise=rise)
    if estimated and fps is not None:
        ar1_gamma(1.0, fps)
    if bin_frames is not None and refine is None and split is None:
        raise ValueError('--bin-frames needs --refine or --split: it bins the frames those passes correlate')
    if bin_frames is not None and not 1 <= bin_frames <= 64:
        raise ValueError('--bin-frames averages B consecutive frames, B in [1, 64], not %d' % bin_frames)
    if detrend is not None and refine is None and split is None and merge is None:
        raise ValueError('--detrend needs --refine or --split (or --merge): it detrends the correlations those passes form')
    if detrend is not None and not 2 <= detrend <= 4096:
        raise ValueError('--detrend correlates within segments of L frames, L in [2, 4096], not %d' % detrend)
    if merge is not None and merge != merge:
        raise ValueError('--merge joins ROIs whose traces correlate at THR or above: THR must be a number, not NaN')
    if drop_artefacts is not None and not drop_artefacts > 0:
        raise ValueError('--drop-artefacts flags frames beyond K scaled median absolute deviations, K > 0, not %r' % (drop_artefacts,))
    if overlap not in ('keep', 'exclude', 'demix'):
        raise ValueError('--overlap is keep, exclude or demix, not %r' % (overlap,))
    if overlap != 'keep' and weighted is None:
        raise ValueError('--overlap needs --weighted')
    if overlap == 'demix' and dff is not None:
        raise ValueError('--overlap demix gives float64 coefficients, --dff takes integer sums: not together')
    if weighted is not None and weighted != weighted:
        raise ValueError('--weighted drops pixels whose correlation is below FLOOR: FLOOR must be a number, not NaN')
    if not 0 <= merge_dist <= 16:
        raise ValueError('--merge-dist is the largest gap between two fragments in pixels, D in [0, 16], not %d' % merge_dist)
    known = 'fine_shifts' if subpixel else 'shifts'
    unit = 16 if subpixel else 1
    dspaths = nf_find_hdf5(dataset_name)
    shifts, offsets, templates, keeps = {}, {}, {}, {}

    def moves(p):
        # the keywords of every reader of the recording: the known shifts and the scan-phase offset
        return {known: shifts.get(p), 'bidi': offsets.get(p, 0)}

    def kept(p):
        # and of every reader that correlates: the frames --drop-artefacts leaves out
        return dict(moves(p), keep=keeps.get(p))

    def n_read(p):
        # the frames those readers see: b and L count kept frames
        return int(keeps[p].sum()) if p in keeps else _n_frames(p)
    if bidi is not None:
        for dspath in dspaths:
            offsets[dspath], totals = estimate_bidi_device(dspath, max_offset=bidi, frames=200)
            ranked = sorted(totals)
            logger.info('%s: scan-phase offset %+d of the odd lines (searched within +-%d over the first 200 frames): total %d, '
                        'runner-up %d, gap %d' % (dspath, offsets[dspath], bidi, ranked[0], ranked[min(1, len(ranked) - 1)],
                                                  ranked[min(1, len(ranked) - 1)] - ranked[0]))
    if register is not None:
        for dspath in dspaths:
            shifts[dspath], tmpl = estimate_shifts_device(dspath, max_shift=register, blocks=blocks, max_dev=max_dev, subpixel=subpixel,
                                                          coarse=coarse, bidi=offsets.get(dspath, 0))
            templates[dspath] = tmpl
            logger.info('%s: registered within +-%d%s%s%s, largest |dy|, |dx| = %g, %g, valid rectangle %r' % (
                dspath, register, '' if coarse is None else ' (wide search, binned %d x %d)' % (coarse, coarse), '' if blocks is None else ' in %d x %d blocks within +-%d of that' % (blocks + (max_dev,)),
                ', refined to 1/16 pixel' if subpixel else '',
                np.abs(shifts[dspath][..., 0]).max() / unit, np.abs(shifts[dspath][..., 1]).max() / unit,
                valid_rectangle(shifts[dspath], tmpl.shape, fine=subpixel, bidi=offsets.get(dspath, 0))))
    if drop_artefacts is not None:
        from deep_calcium_amd.series import _open_series
        for dspath in dspaths:
            if dspath not in templates:              # no registration: the rounded mean of the first 200 frames, lines corrected
                frames, close = _open_series(dspath, 'series/raw')
                try:
                    templates[dspath] = make_template(np.asarray(frames[:200]), max_shift=0, iterations=0, bidi=offsets.get(dspath, 0))
                finally:
                    frames = None
                    close()
            tmpl = templates[dspath]
            rect = valid_rectangle(shifts[dspath], tmpl.shape, fine=subpixel, bidi=offsets.get(dspath, 0)) if dspath in shifts else None
            mean, corr = frame_quality_device(dspath, template=tmpl, rect=rect, **moves(dspath))
            keeps[dspath] = flag_frames(mean, corr, k=drop_artefacts)
            flagged = np.flatnonzero(~keeps[dspath])
            logger.info('%s: %d of %d frames flagged as artefacts at K = %g (scored over %s; mean %g +- %g, corr %g): %s' % (
                dspath, len(flagged), len(mean), drop_artefacts, 'the whole frame' if rect is None else 'the valid rectangle %r' % (rect,),
                np.median(mean), 1.4826 * np.median(np.abs(mean - np.median(mean))), np.median(corr),
                ' '.join(str(t) for t in flagged) or 'none'))
    if register is not None or bidi is not None or drop_artefacts is not None:
        model = UNet2DSummary(cpdir=checkpoints_dir, series_summary_func=lambda p: summarize_series_device(p, kind='mean', **kept(p)))
    else:
        model = UNet2DSummary(cpdir=checkpoints_dir)
    Mp, names = model.predict(dspaths, model_path=model_path, window_shape=(512, 512), save=False, augmentation=True)
    for dspath, mp, name in zip(dspaths, Mp, names):
        mask = np.asarray(mp).round().astype(np.uint8)
        if not mask.any():
            logger.info('%s: no neurons predicted, no traces file.' % name)
            continue
        if bin_frames is not None:
            T = n_read(dspath)
            logger.info('%s: the refinement and the split read the means of %d consecutive frames: %d binned frames of %d'
                        % (name, bin_frames, T // bin_frames, T))
        if detrend is not None:
            n = n_read(dspath) // (bin_frames or 1)
            plan = detrend_plan(n, detrend)
            logger.info('%s: the refinement and the split correlate within segments of L = %d frames: %d segments over %d frames, L_last = %d'
                        % (name, detrend, len(plan), n, plan[-1][1]))
        if refine is not None:
            corr, coords, inside = roi_footprints_device(dspath, mask, halo=halo, bin_frames=bin_frames, detrend_frames=detrend, **kept(dspath))
            rois, kept_rois = refine_rois(coords, corr, mask.shape, threshold=refine)
            before = [set(map(tuple, c[i].tolist())) for c, i in zip(coords, inside)]
            after = dict((r, set(map(tuple, c.tolist()))) for r, c in zip(kept_rois, rois))
            logger.info('%s: refined at corr >= %g (halo %d): %d of %d ROIs dropped, %d pixels removed, %d added' % (
                name, refine, halo, len(coords) - len(kept_rois), len(coords),
                sum(len(b - after.get(r, set())) for r, b in enumerate(before)),
                sum(len(after[r] - before[r]) for r in kept_rois)))
            if not rois:
                logger.info('%s: no ROI survives the refinement, no traces file.' % name)
                continue
            mask = rois
        if split is not None:
            rois, origin, gaps = split_rois_device(dspath, mask, min_gap=split, min_area=min_area, bin_frames=bin_frames, detrend_frames=detrend,
                                                   **kept(dspath))
            before = int(np.count_nonzero(mask)) if isinstance(mask, np.ndarray) else sum(len(r) for r in mask)
            logger.info('%s: split at gap >= %g (min area %d): %d of %d ROIs split, %d pixels dropped' % (
                name, split, min_area, len(rois) - len(gaps), len(gaps), before - sum(len(r) for r in rois)))
            mask = rois
        if merge is not None:
            rois, origin, pairs, corr = merge_rois_device(dspath, mask, max_dist=merge_dist, threshold=merge, detrend_frames=detrend,
                                                          **kept(dspath))
            logger.info('%s: merged at trace corr >= %g (within %d pixels%s): %d candidate pairs, %d accepted, %d ROIs -> %d' % (
                name, merge, merge_dist, '' if detrend is None else ', within segments of L = %d of all %d frames' % (detrend, n_read(dspath)),
                len(pairs), int(np.count_nonzero(corr >= merge)), sum(len(o) for o in origin), len(rois)))
            mask = rois
        if weighted is not None:
            corr, coords, inside = roi_footprints_device(dspath, mask, halo=0, bin_frames=bin_frames, detrend_frames=detrend, **kept(dspath))
            rois, weights, kept_rois = footprint_weights(coords, corr, inside=inside, floor=weighted)
            if not rois:
                logger.info('%s: no pixel reaches corr >= %g, no traces file.' % (name, weighted))
                continue
            frame_shape = np.asarray(mp).shape[-2:]
            found = shared_pixels(rois, frame_shape)
            logger.info('%s: weighted at corr >= %g: %d of %d ROIs kept, %d pixels dropped, %d shared pixels found (--overlap %s)' % (
                name, weighted, len(kept_rois), len(coords), sum(int(i.sum()) for i in inside) - sum(len(r) for r in rois), found, overlap))
            if overlap == 'exclude':
                rois, weights, kept_rois = exclude_overlap(rois, frame_shape, weights)
                if not rois:
                    logger.info('%s: every pixel is shared, no traces file.' % name)
                    continue
            if dff is not None:
                tr = dff_traces_device(dspath, rois, dff, percentile=percentile, neuropil=neuropil, weights=weights, **moves(dspath))
            elif overlap == 'demix':
                tr = weighted_traces_device(dspath, rois, weights, kind='zscore' if kind == 'zscore' else 'demix', overlap='demix', **moves(dspath))
            else:
                tr = weighted_traces_device(dspath, rois, weights, kind=kind, **moves(dspath))
        elif dff is not None:
            tr = dff_traces_device(dspath, mask, dff, percentile=percentile, neuropil=neuropil, **moves(dspath))
        else:
            tr = extract_traces_device(dspath, mask, kind=kind, **moves(dspath))
        extra = None
        if spike_rise == 'auto':
            dyn = TraceDynamicsAR2(tr)
            sigma = dyn.result('noise')
            _, status, (g_pool, r_pool) = pick_roots(dyn.result('g12_raw'))
            if spike_constrain is not None:
                dec = TraceDeconvolver(dyn.traces_device, g_pool, rise=r_pool, constrain=spike_constrain, sigma=dyn.result_device('noise'), **base_kw)
            else:
                dec = TraceDeconvolver(dyn.traces_device, g_pool, rise=r_pool, s_min=spike_k * sigma, **base_kw)
            extra = dict(calcium=dec.result('calcium'), deconvolved=dec.result('spikes'))
            events = (extra['deconvolved'] > 0).sum(1)
            g1, g2 = ar2_coefficients(g_pool, r_pool)
            logger.info('%s: decay and rise estimated from the traces (--deconvolve auto --spike-rise auto, %d lags): pooled d = %.6f, r = %.6f%s, '
                        'g1 = %.6f, g2 = %.6f; the response to one spike peaks at frame %d; status fine / complex / no rise / too slow / '
                        'undefined = %d / %d / %d / %d / %d; s_min = %g sigma_hat, median sigma_hat %.4g: events per ROI min / median / max = '
                        '%d / %g / %d' % (
                            name, dyn.lags, g_pool, r_pool,
                            '' if fps is None else ' (tau %.4g s, tau_rise %.4g s at %g frames/s)' % (ar1_tau(g_pool, fps), ar1_tau(r_pool, fps), fps),
                            g1, g2, ar2_peak(g_pool, r_pool), int((status == 0).sum()), int((status == 1).sum()), int((status == 2).sum()),
                            int((status == 3).sum()), int((status == 4).sum()), 0.0 if spike_constrain == 'lam' else spike_k,
                            float(np.median(sigma)), int(events.min()), float(np.median(events)), int(events.max())))
        elif estimated:
            dyn = TraceDynamics(tr)
            sigma = dyn.result('noise')
            g_each, status, g_pool = pick_gamma(dyn.result('g_raw'))
            if spike_constrain is not None:
                dec = TraceDeconvolver(dyn.traces_device, g_pool if deconvolve == 'auto' else g_each, constrain=spike_constrain,
                                       sigma=dyn.result_device('noise'), **base_kw)
            else:
                dec = TraceDeconvolver(dyn.traces_device, g_pool if deconvolve == 'auto' else g_each, s_min=spike_k * sigma, **base_kw)
            extra = dict(calcium=dec.result('calcium'), deconvolved=dec.result('spikes'))
            events = (extra['deconvolved'] > 0).sum(1)
            logger.info('%s: decay estimated from the traces (--deconvolve %s): pooled g = %.6f%s, per trace min / median / max = %.6f / %.6f / '
                        '%.6f%s; status fine / raised / lowered / replaced = %d / %d / %d / %d; s_min = %g sigma_hat, median sigma_hat %.4g: '
                        'events per ROI min / median / max = %d / %g / %d' % (
                            name, deconvolve, g_pool, '' if fps is None else ' (tau %.4g s at %g frames/s)' % (ar1_tau(g_pool, fps), fps),
                            float(g_each.min()), float(np.median(g_each)), float(g_each.max()),
                            '' if fps is None else ' (tau %.4g / %.4g / %.4g s)' % tuple(ar1_tau(float(v), fps) for v in (g_each.min(), np.median(g_each), g_each.max())),
                            int((status == 0).sum()), int((status == 1).sum()), int((status == 2).sum()), int((status == 3).sum()),
                            0.0 if spike_constrain == 'lam' else spike_k, float(np.median(sigma)), int(events.min()), float(np.median(events)),
                            int(events.max())))
        elif g is not None:
            sigma = trace_noise(tr)
            dec = (TraceDeconvolver(tr, g, s_min=spike_k * sigma, **base_kw) if spike_constrain is None else
                   TraceDeconvolver(tr, g, constrain=spike_constrain, **base_kw))
            extra = dict(calcium=dec.result('calcium'), deconvolved=dec.result('spikes'))
            events = (extra['deconvolved'] > 0).sum(1)
            logger.info('%s: deconvolved with g = %.6f (tau %g s at %g frames/s), s_min = %g sigma_hat, median sigma_hat %.4g: '
                        'events per ROI min / median / max = %d / %g / %d' % (name, g, deconvolve, fps, 0.0 if spike_constrain == 'lam' else spike_k,
                                                                              float(np.median(sigma)), int(events.min()), float(np.median(events)),
                                                                              int(events.max())))
            if rise is not None:
                g1, g2 = ar2_coefficients(g, rise)
                logger.info('%s: AR(2) (--spike-rise %g s): d = %.6f, r = %.6f, g1 = %.6f, g2 = %.6f; the response to one spike peaks at frame %d'
                            % (name, spike_rise, g, rise, g1, g2, ar2_peak(g, rise)))
        if extra is not None and spike_constrain is not None:
            found, st = dec.result('param'), dec.result('status')
            ratio = found[sigma > 0] / sigma[sigma > 0] if (sigma > 0).any() else np.zeros(1)
            logger.info('%s: %s searched per trace until the residual equals the noise (--spike-constrain: the s_min = K sigma_hat of the line '
                        'above was not used): %s / sigma_hat min / median / max = %.3g / %.3g / %.3g; status bracketed / zero / never bracketed = %d / %d / %d'
                        % (name, spike_constrain, spike_constrain, float(ratio.min()), float(np.median(ratio)), float(ratio.max()),
                           int((st == 0).sum()), int((st == 1).sum()), int((st == 2).sum())))
        if extra is not None and spike_baseline is not None:
            b = dec.result('baseline')
            ratio = b[sigma > 0] / sigma[sigma > 0] if (sigma > 0).any() else np.zeros(1)
            logger.info('%s: a baseline per trace in the deconvolution (--spike-baseline %s): baseline / sigma_hat min / median / max = '
                        '%.3g / %.3g / %.3g' % (name, spike_baseline, float(ratio.min()), float(np.median(ratio)), float(ratio.max())))
        out = write_traces_dataset('%s/%s_traces.hdf5' % (model.cpdir, name), tr, name, extra=extra)
        logger.info('%s: %d traces of %d frames -> %s' % (name, tr.shape[0], tr.shape[1], out))
        logger.info('spikes: python examples/spikes/unet1d.py predict %s --model unet1d_model.hdf5' % out)


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description='CLI for UNet2DS model.')
    sp = ap.add_subparsers(title='actions', description='Choose an action.')
    sp_trn = sp.add_parser('train', help='CLI for training.')
    sp_trn.set_defaults(which='train')
    sp_trn.add_argument('dataset_name', help='dataset name', default='all_train', type=str)
    sp_trn.add_argument('-m', '--model_path', help='path to model')
    sp_trn.add_argument('-c', '--checkpoints_dir', help='checkpoint directory', default=CHECKPOINTS_DIR)
    sp_trn.add_argument('--nb_steps', help='training batches per epoch', default=100, type=int)
    sp_trn.add_argument('--nb_epochs', help='epochs', default=10, type=int)
    sp_eva = sp.add_parser('evaluate', help='CLI for evaluation.')
    sp_eva.set_defaults(which='evaluate')
    sp_eva.add_argument('dataset_name', help='dataset name', default='all_train', type=str)
    sp_eva.add_argument('-m', '--model_path', help='path to model', required=True)
    sp_eva.add_argument('-c', '--checkpoints_dir', help='checkpoint directory', default=CHECKPOINTS_DIR)
    sp_prd = sp.add_parser('predict', help='CLI for prediction.')
    sp_prd.set_defaults(which='predict')
    sp_prd.add_argument('dataset_name', help='dataset name', default='all', type=str)
    sp_prd.add_argument('-m', '--model_path', help='path to model', required=True)
    sp_prd.add_argument('-c', '--checkpoints_dir', help='checkpoint directory', default=CHECKPOINTS_DIR)
    sp_trc = sp.add_parser('traces', help='CLI for ROI traces of predicted neurons.')
    sp_trc.set_defaults(which='traces')
    sp_trc.add_argument('dataset_name', help='dataset name', default='all', type=str)
    sp_trc.add_argument('-m', '--model_path', help='path to model', required=True)
    sp_trc.add_argument('-c', '--checkpoints_dir', help='checkpoint directory', default=CHECKPOINTS_DIR)
    sp_trc.add_argument('--kind', help='what a trace holds', default='mean', choices=('sum', 'mean', 'zscore'))
    sp_trc.add_argument('--register', help='register the raw frames first, within +-S pixels (default 8)', nargs='?', const=8, default=None,
                        type=int, metavar='S')
    sp_trc.add_argument('--blocks', help='with --register: piecewise-rigid, one shift per block of a By x Bx grid (e.g. 4x4)', default=None,
                        type=_blocks_arg, metavar='ByxBx')
    sp_trc.add_argument('--max-dev', help='with --blocks: a block may deviate from the rigid shift by +-D pixels (default 3)', default=3,
                        type=int, metavar='D', dest='max_dev')
    sp_trc.add_argument('--coarse', help='with --register: the wide search, a coarse shift on frames binned C x C first; S may then reach 16 C',
                        default=None, type=int, choices=(2, 4, 8), metavar='C')
    sp_trc.add_argument('--subpixel', help='with --register: refine every shift to 1/16 pixel and interpolate the frames', action='store_true')
    sp_trc.add_argument('--bidi', help='undo the scan-phase offset of the odd lines first: searched within +-P pixels (default 8, at most 16) '
                        'over the first 200 frames', nargs='?', const=8, default=None, type=int, metavar='P')
    sp_trc.add_argument('--dff', help='write dF/F against a rolling-percentile baseline over WINDOW frames (odd) instead of --kind', default=None,
                        type=int, metavar='WINDOW')
    sp_trc.add_argument('--percentile', help='with --dff: the integer percentile of the baseline (default 8)', default=8, type=int, metavar='Q')
    sp_trc.add_argument('--neuropil', help='with --dff: subtract WEIGHT times the trace of the ring INNER < distance <= OUTER (e.g. 2,12,0.7)',
                        default=None, type=_neuropil_arg, metavar='INNER,OUTER,WEIGHT')
    sp_trc.add_argument('--deconvolve', help='with --dff: deconvolve the dF/F traces (non-negative AR(1), no trained model); TAU: the indicator '
                        'decay time in seconds (needs --fps); auto: the decay is estimated from the traces, the pooled median serves all; each: '
                        'every trace gets its own estimate; writes `calcium` and `deconvolved` beside `traces`', default=None, type=_deconvolve_arg,
                        metavar='auto|each|TAU')
    sp_trc.add_argument('--fps', help='with --deconvolve: the frame rate of the recording in frames per second', default=None, type=float, metavar='F')
    sp_trc.add_argument('--spike-k', help='with --deconvolve: the smallest spike allowed, in units of every trace\'s noise (default 3)', default=3.0,
                        type=float, metavar='K', dest='spike_k')
    sp_trc.add_argument('--spike-rise', help='with --deconvolve TAU: the rise time of the indicator in seconds; the model is then AR(2), with the '
                        'roots exp(-1 / (TAU F)) and exp(-1 / (TAU_RISE F)); auto (with --deconvolve auto): both roots are estimated from the '
                        'traces and the pooled pair serves all', default=None, type=_rise_arg, metavar='auto|TAU_RISE', dest='spike_rise')
    sp_trc.add_argument('--spike-constrain', help='with --deconvolve, instead of --spike-k: search s_min (for events) or lam (for a denoised calcium) '
                        'per trace until the residual equals the trace noise', default=None, choices=('s_min', 'lam'), dest='spike_constrain')
    sp_trc.add_argument('--spike-baseline', help='with --deconvolve: fit one constant per trace inside the deconvolution (fit; recommended with '
                        '--spike-constrain), or take VALUE off every trace (not with --spike-constrain)', default=None, type=_baseline_arg,
                        metavar='fit|VALUE', dest='spike_baseline')
    sp_trc.add_argument('--refine', help='refine every ROI by its footprint map first: keep the pixels whose correlation with the trace is >= THR',
                        default=None, type=float, metavar='THR')
    sp_trc.add_argument('--halo', help='with --refine: how far beyond an ROI, in pixels, its footprint map reaches (0..16, default 2)', default=2,
                        type=int, metavar='N')
    sp_trc.add_argument('--split', help='split every ROI whose pixels form two groups that correlate more within than across by GAP (default 0.1)',
                        nargs='?', const=0.1, default=None, type=float, metavar='GAP')
    sp_trc.add_argument('--min-area', help='with --split: the fewest pixels a part may have (default 8)', default=8, type=int, metavar='N',
                        dest='min_area')
    sp_trc.add_argument('--bin-frames', help='with --refine / --split: correlate the means of B consecutive frames (1..64) instead of single frames',
                        default=None, type=int, metavar='B', dest='bin_frames')
    sp_trc.add_argument('--detrend', help='with --refine / --split / --merge: correlate within segments of L frames (2..4096; binned frames with --bin-frames) and pool them',
                        default=None, type=int, metavar='L')
    sp_trc.add_argument('--merge', help='merge neighbouring ROIs whose traces correlate at THR or above (default 0.8) into one; --detrend applies',
                        nargs='?', const=0.8, default=None, type=float, metavar='THR')
    sp_trc.add_argument('--merge-dist', help='with --merge: the largest distance in pixels between two ROIs that may be merged (0..16, default 2)',
                        default=2, type=int, metavar='D', dest='merge_dist')
    sp_trc.add_argument('--drop-artefacts', help='score every frame first and leave artefact frames (a flash, a gated PMT, a z-jump: mean or template '
                        'correlation beyond K scaled MADs, default 8) out of the summary, --refine, --split and --merge; the traces keep every frame',
                        nargs='?', const=8.0, default=None, type=float, metavar='K', dest='drop_artefacts')
    sp_trc.add_argument('--weighted', help='weight every pixel of the final ROIs by its correlation with its ROI\'s trace (one more footprint pass; '
                        'pixels below FLOOR, default 0, are dropped) and write weighted traces; with --dff the weights are used there',
                        nargs='?', const=0.0, default=None, type=float, metavar='FLOOR')
    sp_trc.add_argument('--overlap', help='with --weighted: pixels that two ROIs share count for both (keep), are dropped (exclude) or are '
                        'demixed by least squares (demix: float64 coefficients; not with --dff)', default='keep', choices=('keep', 'exclude', 'demix'))
    args = vars(ap.parse_args())
    if 'which' not in args:
        ap.error('choose an action: train, evaluate, predict or traces')
    if args['which'] == 'traces' and args['overlap'] == 'demix' and args['dff'] is not None:
        ap.error('--overlap demix gives float64 coefficients, --dff takes integer sums: not together')
    if args['which'] == 'traces' and args['deconvolve'] is not None and args['dff'] is None:
        ap.error('--deconvolve needs --dff: the deconvolution has no baseline term')
    if args['which'] == 'traces' and args['deconvolve'] is not None and not isinstance(args['deconvolve'], str) and args['fps'] is None:
        ap.error('--deconvolve needs --fps')
    if args['which'] == 'traces' and args['spike_rise'] == 'auto':
        if args['deconvolve'] != 'auto':
            ap.error('--spike-rise auto estimates both roots, pooled over the traces: it needs --deconvolve auto')
        if args['spike_baseline'] == 'fit':
            ap.error('--spike-baseline fit is not built for AR(2) (--spike-rise)')
    elif args['which'] == 'traces' and args['spike_rise'] is not None:
        if args['deconvolve'] is None or isinstance(args['deconvolve'], str):
            ap.error('--spike-rise needs --deconvolve TAU: estimating the decay (auto, each) is not built for AR(2)')
        if args['spike_baseline'] == 'fit':
            ap.error('--spike-baseline fit is not built for AR(2) (--spike-rise)')
    if args['which'] == 'traces' and args['spike_constrain'] is not None:
        if any(a == '--spike-k' or a.startswith('--spike-k=') for a in sys.argv[1:]):
            ap.error('--spike-constrain searches the threshold: not together with --spike-k')
        if args['deconvolve'] is None:
            ap.error('--spike-constrain needs --deconvolve')
    if args['which'] == 'traces' and args['spike_baseline'] is not None:
        if args['deconvolve'] is None:
            ap.error('--spike-baseline needs --deconvolve')
        if args['spike_baseline'] != 'fit' and args['spike_constrain'] is not None:
            ap.error('--spike-baseline VALUE cannot go with --spike-constrain: the search fits the baseline (fit) or has none')
    if args['which'] == 'traces' and args['overlap'] != 'keep' and args['weighted'] is None:
        ap.error('--overlap needs --weighted')
    f = {'train': training, 'evaluate': evaluation, 'predict': prediction, 'traces': traces}[args.pop('which')]
    f(**args)
