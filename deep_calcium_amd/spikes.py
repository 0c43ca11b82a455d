"""Spike inference on the device: the reference's UNet1DSegmentation (models/spikes/unet_1d_segmentation.py:177-459), predict only.

The last step of the pipeline recording -> summary image (series.py) -> mask (UNet2DSummary.predict) -> traces (traces.py) ->
spikes: a dataset file of the spikes model's schema (:182-187: attribute `name`, dataset `traces` (no. ROIs, no. frames)) and a
Keras model file of unet1d (:49-148) in, one uint8 (no. ROIs, no. frames) spike segmentation per dataset out.

    model = UNet1DSegmentation(cpdir)
    spikes, names = model.predict(['neurofinder.00.00_traces.hdf5'], 'unet1d_model.hdf5')       # the reference's call (:422-459)
    p = model.predict_proba(traces, 'unet1d_model.hdf5')                                        # (R,T) normalised -> float32 (R,T)

What differs from the reference, stated:
  * fit() is not covered by THIS class: it raises NotImplementedError.  Training the 1-D network (:217-420) lives in
    spikes_fit.TrainableUNet1DSegmentation, a subclass with the reference's fit() signature.
  * Trace length.  The reference graph exists only for T % 16 == 0 (four poolings; Keras fails at the first concatenate
    otherwise).  Here a trace of ANY T >= 1 is extended on the right with zeros -- the mean of a z-scored trace -- to the next
    multiple of 16 and the output is cropped to T.  This has no reference counterpart; for T % 16 == 0 nothing is padded.
  * A trace that is constant in time normalises to zeros (numpy gives NaN and the reference's asserts :165-166 fail): the
    convention of traces.py.
  * A trace's probabilities are bit-identical however the traces are batched (`batch`, the order, alone or together).
  * The loaded model is kept while its file is unchanged (the reference re-reads it per dataset, :453-454).

Importing this module needs neither torch nor the GPU; predicting does (there is no CPU fallback).
"""
import os

import numpy as np

from . import hdf5_min


def _open_members(dspath):
    """-> (attrs dict, {name: array getter}) of a dataset file: HDF5 through hdf5_min, or the .npz write_traces_dataset makes."""
    if str(dspath).endswith('.npz'):
        z = np.load(dspath, allow_pickle=False)
        return ({'name': str(z['name'])} if 'name' in z.files else {}), z
    f = hdf5_min.File(dspath)
    attrs = {}
    for k, v in f.attrs.items():
        attrs[k] = v.decode('utf8') if isinstance(v, (bytes, np.bytes_)) else v
    return attrs, f


def _close(f):
    if hasattr(f, 'close'):
        f.close()


def get_dataset_attrs(dspath):
    """:151-155."""
    attrs, f = _open_members(dspath)
    _close(f)
    return attrs


def normalize_traces(traces):
    """:162-164 in float64: (traces - mean) / std along time, population std.  A trace constant in time becomes zeros."""
    traces = np.asarray(traces, np.float64)
    if traces.ndim != 2 or traces.shape[0] < 1 or traces.shape[1] < 1:
        raise ValueError('traces must be a non-empty (R,T) matrix, not %r' % (traces.shape,))
    m = np.mean(traces, axis=1, keepdims=True)
    s = np.std(traces, axis=1, keepdims=True)
    flat = s[:, 0] == 0
    s[flat] = 1.
    out = (traces - m) / s
    out[flat] = 0.
    return out


def get_dataset_traces(dspath):
    """:158-167: the file's `traces`, normalised per trace."""
    _, f = _open_members(dspath)
    try:
        if 'traces' not in f:
            raise ValueError('%s has no `traces` (the spikes model\'s schema: attribute name, dataset traces (R,T))' % dspath)
        tr = f['traces']
        return normalize_traces(tr.read() if hasattr(tr, 'read') else tr)      # read() copies: nothing keeps the mapping
    finally:
        _close(f)


def unet1d_hip(weights, nb_filters_base=32, margin=4, device=None):
    """The default net_builder_func: the HIP inference engine of the unet1d graph."""
    from .unet1d import UNet1DEngine
    return UNet1DEngine(weights, nb_filters_base, margin, device=device)


def _check_batch(batch):
    if isinstance(batch, bool) or not isinstance(batch, (int, np.integer)) or batch < 1:
        raise ValueError('batch must be an integer >= 1 (traces per forward), not %r' % (batch,))
    return int(batch)


def _check_threshold(threshold):
    try:
        t = float(threshold)
    except (TypeError, ValueError):
        raise ValueError('threshold must be a number in [0, 1], not %r' % (threshold,))
    if not 0. <= t <= 1.:
        raise ValueError('threshold must be a number in [0, 1], not %r' % (threshold,))
    return t


def _check_traces(traces):
    traces = np.asarray(traces)
    if traces.ndim != 2 or traces.dtype.kind not in 'fiu' or traces.shape[0] < 1 or traces.shape[1] < 1:
        raise ValueError('traces must be a non-empty numeric (R,T) matrix, not %s %r' % (traces.dtype, traces.shape))
    if not np.all(np.isfinite(traces)):
        raise ValueError('traces hold NaN or inf')
    return traces


class UNet1DSegmentation(object):
    """Trace segmentation wrapper with the reference's constructor (:202-215); dataset_spikes_func is accepted and kept (only
    training reads it)."""

    _CACHE_MAX = 2

    def __init__(self, cpdir=None, dataset_attrs_func=get_dataset_attrs, dataset_traces_func=get_dataset_traces,
                 dataset_spikes_func=None, net_builder_func=unet1d_hip):
        if cpdir is None:
            from .nf_datasets import default_dirs
            cpdir = '%s/spikes_unet1d' % default_dirs()[1]
        self.cpdir = cpdir
        self.dataset_attrs_func = dataset_attrs_func
        self.dataset_traces_func = dataset_traces_func
        self.dataset_spikes_func = dataset_spikes_func
        self.net_builder_func = net_builder_func
        self.model_reads = 0                       # how often a model file was parsed (the cache's witness)
        if not os.path.exists(self.cpdir):
            os.makedirs(self.cpdir)

    def fit(self, *args, **kwargs):
        raise NotImplementedError('UNet1DSegmentation.fit: training the 1-D network is not covered by this package (inference '
                                  'only: predict / predict_proba); train with the reference and load its model file here')

    def _model(self, model_path, margin=4):
        st = os.stat(model_path)
        key = (os.path.realpath(model_path), st.st_mtime_ns, st.st_size, int(margin))
        cache = self.__dict__.setdefault('_models', [])
        for i, (k, m) in enumerate(cache):
            if k == key:
                cache.append(cache.pop(i))
                return m
        from .keras_io import read_keras_unet1d
        m = read_keras_unet1d(model_path, margin=margin)
        self.model_reads += 1
        eng = self.net_builder_func(m['weights'], nb_filters_base=m['config']['nb_filters_base'], margin=m['config']['margin'])
        cache.append((key, eng))
        del cache[:-self._CACHE_MAX]
        return eng

    def _proba_device(self, traces, model_path, batch, margin):
        """(R,T) normalised host matrix -> float32 (R,T) on the host; `batch` traces per forward, T zero-extended to 16k."""
        eng = self._model(model_path, margin)
        import torch
        R, T = traces.shape
        Tp = (T + 15) // 16 * 16
        x = np.zeros((R, Tp), np.float32)
        x[:, :T] = traces
        xd = torch.from_numpy(x).to(eng.device)
        outs = [eng.forward(xd[a:a + batch]) for a in range(0, R, batch)]
        return torch.cat(outs, 0)[:, :T].cpu().numpy()

    def predict_proba(self, traces, model_path, batch=32, margin=4):
        """traces: (R,T), already normalised.  `margin` only matters for a weights-only model file (no model_config)."""
        batch = _check_batch(batch)
        traces = _check_traces(traces)
        if not os.path.isfile(model_path):
            raise ValueError('model file %r does not exist' % (model_path,))
        return self._proba_device(traces, model_path, batch, margin)

    def predict(self, dataset_paths, model_path, batch=32, threshold=0.5):
        """:422-459.  -> (spikes_pred_all: one uint8 (R,T) matrix of p > threshold per dataset, names_all)."""
        batch = _check_batch(batch)
        threshold = _check_threshold(threshold)
        if isinstance(dataset_paths, (str, bytes)) or not hasattr(dataset_paths, '__iter__'):
            raise ValueError('dataset_paths must be a list of dataset files, not %r' % (dataset_paths,))
        dataset_paths = list(dataset_paths)
        for p in list(dataset_paths) + [model_path]:
            if not os.path.isfile(p):
                raise ValueError('file %r does not exist' % (p,))
        spikes_pred_all, names_all = [], []
        for p in dataset_paths:
            attrs = self.dataset_attrs_func(p)
            names_all.append(attrs['name'])
            traces = _check_traces(self.dataset_traces_func(p))
            proba = self._proba_device(traces, model_path, batch, 4)
            spikes_pred_all.append((proba > threshold).astype(np.uint8))
        return spikes_pred_all, names_all


def predict_spikes_device(path_or_traces, model_path, batch=32, threshold=0.5, cpdir=None, proba=False):
    """One call: a dataset file (-> what predict() gives for it: uint8 (R,T)) or an (R,T) matrix of normalised traces.
    proba=True returns the float32 probabilities instead of p > threshold."""
    batch = _check_batch(batch)
    threshold = _check_threshold(threshold)
    import tempfile
    model = UNet1DSegmentation(cpdir if cpdir is not None else tempfile.gettempdir())
    if isinstance(path_or_traces, (str, bytes, os.PathLike)):
        if not os.path.isfile(path_or_traces):
            raise ValueError('file %r does not exist' % (path_or_traces,))
        traces = model.dataset_traces_func(path_or_traces)
    else:
        traces = path_or_traces
    p = model.predict_proba(traces, model_path, batch=batch)
    return p if proba else (p > threshold).astype(np.uint8)
