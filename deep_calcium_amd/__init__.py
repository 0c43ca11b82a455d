"""deep_calcium_amd: the UNet2DS hot path of alexklibisz/deep-calcium, MI355X-native.

    from deep_calcium_amd import UNet2DSummary, unet_hip

`UNet2DSummary` keeps the reference's fit()/predict() surface; `unet_hip` is the drop-in `net_builder_func`.
Every tensor op runs as a hand-written gfx950 HIP kernel behind the C ABI in include/dcunet.h; there is no
CPU fallback (importing is cheap and GPU-free, constructing a model requires the GPU and libdcunet.so).
The public names are resolved on first use (PEP 562): importing a torch-free submodule (`deep_calcium_amd.keras_io`,
`.nf_metrics`, `.layers` -- what the background checkpoint-writer process loads) does not import torch.
"""
import os as _os

__version__ = '0.1.0'

# HIP multiplexes a process's streams onto GPU_MAX_HW_QUEUES hardware queues (default 4).  A data-parallel rank holds more than
# that -- the step's main and weight-gradient streams, the input copy stream, torch.distributed's collective stream, RCCL's own
# per-communicator streams -- and when the weight-gradient stream ends up sharing the main stream's queue the two-stream backward
# serialises (measured in round 6: 17.5 -> 18.2-18.6 ms per step, every launch of the trace on one queue; 17.47 ms with 8 queues, and
# no change for a single-GPU run: 17.41 vs 17.42).  Only a default: an explicit setting wins, and it takes effect only if the HIP
# runtime has not initialised yet (it reads the variable once) -- UNetEngine also makes its side stream first, for that case.
_os.environ.setdefault('GPU_MAX_HW_QUEUES', '8')

_EXPORTS = {
    'model': ('Model', 'Adam', 'Callback', 'CSVLogger', 'ModelCheckpoint', 'ReduceLROnPlateau', 'History', 'unet_hip',
              'load_model_with_new_input_shape', 'metrics_from_sums'),
    'unet2ds': ('UNet2DSummary', 'INVERTIBLE_2D_AUGMENTATIONS', '_ValidationMetricsCB'),
    'nf_metrics': ('nf_mask_metrics',),
    'series': ('SeriesSummarizer', 'summarize_series_device', 'TemporalBinner', 'detrend_plan'),
    'traces': ('RoiTraceExtractor', 'rois_to_csr', 'extract_traces_device', 'write_traces_dataset'),
    'footprints': ('RoiFootprints', 'roi_footprints_device', 'roi_support', 'refine_rois'),
    'roi_pairs': ('RoiPairCorr', 'roi_pair_corr_device', 'split_rois', 'split_rois_device'),
    'merge': ('TracePairCorr', 'roi_neighbours', 'merge_rois', 'merge_rois_device'),
    'frames': ('FrameQuality', 'FrameFilter', 'frame_quality_device', 'flag_frames', 'hold_index'),
    'weighted': ('WeightedTraceExtractor', 'weighted_traces_device', 'footprint_weights', 'exclude_overlap', 'roi_gram', 'demix_traces'),
    'dff': ('TraceBaseline', 'neuropil_rois', 'dff_traces_device'),
    'deconv': ('TraceDeconvolver', 'deconvolve_traces_device', 'ar1_gamma', 'ar1_table', 'ar2_table', 'trace_noise'),
    'dynamics': ('TraceDynamics', 'estimate_ar1_device', 'ar1_tau', 'pick_gamma', 'TraceDynamicsAR2', 'estimate_ar2_device', 'ar2_roots',
                 'pick_roots'),
    'motion': ('MotionCorrector', 'make_template', 'estimate_shifts_device', 'valid_rectangle', 'fine_to_pixels', 'BidiEstimator',
               'pick_bidi', 'estimate_bidi_device'),
    'spikes': ('UNet1DSegmentation', 'predict_spikes_device'),
    'unet1d': ('UNet1DEngine',),
    'unet1d_train': ('UNet1DTrainEngine',),
    'spikes_fit': ('TrainableUNet1DSegmentation', 'get_dataset_spikes', 'fit_spikes_device'),
}
_WHERE = dict((name, mod) for mod, names in _EXPORTS.items() for name in names)
__all__ = sorted(_WHERE)


def __getattr__(name):
    mod = _WHERE.get(name)
    if mod is None:
        raise AttributeError('module %r has no attribute %r' % (__name__, name))
    import importlib
    value = getattr(importlib.import_module('.' + mod, __name__), name)
    globals()[name] = value
    return value


def __dir__():
    return sorted(list(globals()) + list(_WHERE))
