"""Training the spikes model on the device: the reference's UNet1DSegmentation.fit (models/spikes/unet_1d_segmentation.py:217-420).

    model = TrainableUNet1DSegmentation(cpdir)
    history, best_model_path = model.fit(['a_traces.hdf5', 'b_traces.hdf5'])         # the reference's call (:217-219)
    spikes, names = model.predict(['c_traces.hdf5'], best_model_path)               # inherited: spikes.UNet1DSegmentation.predict
    history, best_model_path = fit_spikes_device(paths, cpdir=..., nb_epochs=5)     # one call

TrainableUNet1DSegmentation is a subclass: `UNet1DSegmentation.fit` in spikes.py stays the NotImplementedError its test pins
(tests/test_spikes_api.py), and everything that trains lives here.  Folding the subclass back into the base class is a follow-up.

fit() follows :247-380: the index split of both val_types from numpy's global RNG, the margin max-pooling of the labels once up
front (TensorFlow 'SAME', pool = int(margin) + 1), the _batch_gen sampler with the reference's RNG call sequence (:398-420: one
choice(replace=False) per pass, one randint per window), steps = ceil(n_trn / batch), ONE validation batch of 2 n_val windows, the
per-epoch val_* metrics, ModelCheckpoint(monitor='val_F2', mode='max', save_best_only=True) under the reference's file-name
pattern, CSVLogger, and the final train / validation metrics of the best model.  The network is unet1d_train.UNet1DTrainEngine.

What differs from the reference, stated:
  * The PNG plot callbacks (_SamplePlotCallback, MetricsPlotCallback) are not built.  The one training batch the reference draws
    for its sample plot (:289) is still drawn and dropped, so the sampler's RNG state at the first step is the reference's.
  * A trace exactly shape[0] long gives x0 = 0 (the reference's randint(0, 0) raises); a shorter trace is a ValueError naming
    the dataset.
  * fit() returns (history, best_model_path) as the reference's docstring promises (its code returns nothing); with
    val_type='cross_validate' history is the list of the folds' histories and best_model_path the best model of the fold with
    the highest final validation F2.
  * The time stamp in the checkpoint names is advanced until it is unused: two folds inside one second do not share files.
  * optimizer=None means Adam(0.002), built per call (the reference's default argument is one shared instance).
  * The validation metrics of an epoch are evaluated in batches of `batch` windows.

Every argument error is a ValueError before torch or the library is touched.  Importing this module needs neither.
"""
import glob
import logging
import math
import os
import time

import numpy as np

from .spikes import UNet1DSegmentation, _close, _open_members, get_dataset_attrs, get_dataset_traces, unet1d_hip
from .unet1d_train import METRIC_NAMES, check_train_args

VAL_TYPES = ('random_split', 'cross_validate')


def get_dataset_spikes(dspath):
    """:170-174: the file's `spikes` (R,T), HDF5 through hdf5_min or the .npz write_traces_dataset makes."""
    _, f = _open_members(dspath)
    try:
        if 'spikes' not in f:
            raise ValueError('%s has no `spikes` (training needs the binary spike matrix beside `traces`)' % dspath)
        sp = f['spikes']
        sp = np.asarray(sp.read() if hasattr(sp, 'read') else sp)
    finally:
        _close(f)
    if sp.ndim != 2:
        raise ValueError('%s: `spikes` must be an (R,T) matrix, not %r' % (dspath, sp.shape))
    return sp


def unet1d_train_hip(window_shape, margin=4, nb_filters_base=32, conv_kernel_init='he_normal', prop_dropout_base=0.05, **kw):
    """The default training net_builder_func, with the call signature of the reference's unet1d (:49): the HIP training engine."""
    from .unet1d_train import UNet1DTrainEngine
    return UNet1DTrainEngine(window_shape, nb_filters_base=nb_filters_base, conv_kernel_init=conv_kernel_init,
                             prop_dropout_base=prop_dropout_base, margin=margin, **kw)


def pool_labels(spikes, margin):
    """The error margin applied to the labels (:385-394): MaxPooling(1 x (int(margin) + 1), strides 1, TensorFlow 'SAME' -- the
    smaller pad on the left, padding never wins) of every spike vector.  -> list of float32 vectors."""
    pool = int(margin) + 1
    left, right = (pool - 1) // 2, pool // 2
    out = []
    for s in spikes:
        s = np.asarray(s, np.float32)
        T = len(s)
        p = np.full(T + left + right, -np.inf, np.float32)
        p[left:left + T] = s
        m = p[0:T].copy()
        for k in range(1, pool):
            np.maximum(m, p[k:k + T], out=m)
        out.append(m)
    return out


def split_random(n, prop_trn, prop_val):
    """:335-337, numpy's global RNG: -> (idxs_trn, idxs_val)."""
    idxs = np.random.choice(np.arange(n), n, replace=0)
    return idxs[:int(len(idxs) * prop_trn)], idxs[-1 * int(len(idxs) * prop_val):]


def split_folds(n, nb_folds):
    """:348-350: -> nb_folds disjoint index arrays of int(n / nb_folds)."""
    idxs = np.random.choice(np.arange(n), n, replace=0)
    fsz = int(len(idxs) / nb_folds)
    return [idxs[fsz * k:fsz * k + fsz] for k in range(nb_folds)]


def batch_gen(traces, spikes, shape, batch_size, nb_steps):
    """:396-420 with numpy's global RNG in the reference's call order: per pass of nb_steps batches one
    choice(replace=False) over the traces (cycled), per window one randint(0, len - shape[0]) -- none when len == shape[0]
    (x0 = 0).  `spikes` are already margin-pooled.  Yields (float64 (batch, T), uint8 (batch, T))."""
    T = int(shape[0])
    while True:
        order = np.random.choice(np.arange(len(traces)), len(traces), replace=False)
        k = 0
        for _ in range(nb_steps):
            tb = np.zeros((batch_size, T), dtype=np.float64)
            sb = np.zeros((batch_size, T), dtype=np.uint8)
            for b in range(batch_size):
                idx = order[k % len(order)]
                k += 1
                n = len(spikes[idx])
                x0 = np.random.randint(0, n - T) if n > T else 0
                tb[b] = traces[idx][x0:x0 + T]
                sb[b] = spikes[idx][x0:x0 + T]
            yield tb, sb


def check_fit_args(dataset_paths, shape, error_margin, batch, nb_epochs, val_type, prop_trn, prop_val, nb_folds, keras_callbacks,
                   optimizer):
    """ValueError for every argument fit() cannot run with; touches no file content, torch or the library."""
    if isinstance(dataset_paths, (str, bytes)) or not hasattr(dataset_paths, '__iter__'):
        raise ValueError('dataset_paths must be a list of dataset files, not %r' % (dataset_paths,))
    dataset_paths = list(dataset_paths)
    if not dataset_paths:
        raise ValueError('dataset_paths is empty')
    for p in dataset_paths:
        if not isinstance(p, (str, bytes, os.PathLike)) or not os.path.isfile(p):
            raise ValueError('file %r does not exist' % (p,))
    try:
        margin = float(error_margin)
    except (TypeError, ValueError):
        raise ValueError('error_margin must be a number, not %r' % (error_margin,))
    if not margin >= 0:
        raise ValueError('error_margin must be >= 0, not %r' % (error_margin,))
    check_train_args(shape, 32, 0.05, int(margin))
    for name, v in (('batch', batch), ('nb_epochs', nb_epochs)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError('%s must be an integer >= 1, not %r' % (name, v))
    if val_type not in VAL_TYPES:
        raise ValueError('val_type must be one of %r, not %r' % (VAL_TYPES, val_type))
    if isinstance(nb_folds, bool) or not isinstance(nb_folds, (int, np.integer)) or nb_folds < 2:
        raise ValueError('nb_folds must be an integer > 1, not %r' % (nb_folds,))
    try:
        ok = 0. < float(prop_trn) < 1. and 0. < float(prop_val) < 1. and float(prop_trn) + float(prop_val) == 1.
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('prop_trn and prop_val must be in (0, 1) and add up to 1, not %r and %r' % (prop_trn, prop_val))
    if isinstance(keras_callbacks, (str, bytes)) or not hasattr(keras_callbacks, '__iter__'):
        raise ValueError('keras_callbacks must be a list of callbacks, not %r' % (keras_callbacks,))
    for cb in keras_callbacks:
        if not hasattr(cb, 'on_epoch_end'):
            raise ValueError('keras_callbacks holds %r, which is no callback (no on_epoch_end)' % (cb,))
    if optimizer is not None and not all(hasattr(optimizer, a) for a in ('lr', 'beta_1', 'beta_2', 'epsilon')):
        raise ValueError('optimizer must be None (Adam(0.002)) or an Adam-shaped object with lr, beta_1, beta_2, epsilon; not %r'
                         % (optimizer,))
    return dataset_paths, int(margin)


class TrainableUNet1DSegmentation(UNet1DSegmentation):
    """spikes.UNet1DSegmentation plus fit().  net_builder_func builds the TRAINING network and is called as the reference calls
    its own, net_builder_func(shape, margin=error_margin) (:265); infer_builder_func is what the inherited predict() builds its
    engine with (the base class keeps it as self.net_builder_func)."""

    def __init__(self, cpdir=None, dataset_attrs_func=get_dataset_attrs, dataset_traces_func=get_dataset_traces,
                 dataset_spikes_func=get_dataset_spikes, net_builder_func=unet1d_train_hip, infer_builder_func=unet1d_hip):
        super(TrainableUNet1DSegmentation, self).__init__(cpdir, dataset_attrs_func, dataset_traces_func, dataset_spikes_func,
                                                          infer_builder_func)
        self.train_builder_func = net_builder_func

    def _stamp(self):
        t = int(time.time())
        while glob.glob('%s/%d_*' % (self.cpdir, t)):
            t += 1
        return t

    def _fit_single(self, traces, spikes, idxs_trn, idxs_val, shape, margin, batch, nb_epochs, keras_callbacks, optimizer):
        """:247-316.  -> (history dict, metrics_trn, metrics_val, best_model_path)."""
        from .keras_io import read_keras_unet1d
        from .model import Adam, CSVLogger, History, ModelCheckpoint
        model = self.train_builder_func(shape, margin=margin)
        model.compile(optimizer if optimizer is not None else Adam(0.002))
        tr_trn, sp_trn = [traces[i] for i in idxs_trn], pool_labels([spikes[i] for i in idxs_trn], margin)
        tr_val, sp_val = [traces[i] for i in idxs_val], pool_labels([spikes[i] for i in idxs_val], margin)
        steps_trn = int(math.ceil(len(tr_trn) / float(batch)))
        gen_trn = batch_gen(tr_trn, sp_trn, shape, batch, steps_trn)
        gen_val = batch_gen(tr_val, sp_val, shape, len(tr_val) * 2, 1)
        x_val, y_val = next(gen_val)
        next(gen_trn)                                # the reference's sample-plot batch (:289): drawn, not plotted

        stamp = self._stamp()
        cpt = (self.cpdir, stamp)
        history = History()
        cbs = [history,
               ModelCheckpoint('%s/%d_model_val_F2_{val_F2:3f}_{epoch:03d}.hdf5' % cpt, monitor='val_F2', mode='max', verbose=1,
                               save_best_only=True),
               CSVLogger('%s/%d_metrics.csv' % cpt)] + list(keras_callbacks)
        for cb in cbs:
            if hasattr(cb, 'set_model'):
                cb.set_model(model)
            if hasattr(cb, 'set_params'):
                cb.set_params(dict(epochs=nb_epochs, steps=steps_trn, verbose=1, do_validation=True,
                                   metrics=METRIC_NAMES + ['val_' + n for n in METRIC_NAMES]))
        for cb in cbs:
            cb.on_train_begin({})
        for epoch in range(nb_epochs):
            for cb in cbs:
                cb.on_epoch_begin(epoch, {})
            totals, seen = np.zeros(len(METRIC_NAMES)), 0
            for step in range(steps_trn):
                x, y = next(gen_trn)
                logs = dict(batch=step, size=len(x))
                for cb in cbs:
                    cb.on_batch_begin(step, logs)
                outs = model.train_on_batch(x, y)
                logs.update(zip(METRIC_NAMES, outs))
                for cb in cbs:
                    cb.on_batch_end(step, logs)
                totals += len(x) * np.asarray(outs, np.float64)
                seen += len(x)
            logs = dict(zip(METRIC_NAMES, (float(v) for v in totals / seen)))
            logs.update(('val_' + n, float(v)) for n, v in zip(METRIC_NAMES, model.evaluate(x_val, y_val, batch_size=batch)))
            for cb in cbs:
                cb.on_epoch_end(epoch, logs)
        for cb in cbs:
            cb.on_train_end({})

        # the best serialized model, assuming the newest is the best (:304-307; save_best_only wrote it last)
        model_paths = sorted(glob.glob('%s/%d_model*hdf5' % cpt), key=os.path.getmtime)
        best_model_path = model_paths[-1]
        model.set_weights(read_keras_unet1d(best_model_path, margin=margin)['weights'])
        totals, seen = np.zeros(len(METRIC_NAMES)), 0
        for _ in range(steps_trn):                   # evaluate_generator(gen_trn, steps_trn) (:311)
            x, y = next(gen_trn)
            totals += len(x) * np.asarray(model.evaluate(x, y, batch_size=len(x)), np.float64)
            seen += len(x)
        mt = dict(zip(METRIC_NAMES, (float(v) for v in totals / seen)))
        mv = dict(zip(METRIC_NAMES, (float(v) for v in model.evaluate(x_val, y_val))))
        return history.history, mt, mv, best_model_path

    def fit(self, dataset_paths, shape=(4096,), error_margin=4., batch=20, nb_epochs=20, val_type='random_split', prop_trn=0.8,
            prop_val=0.2, nb_folds=5, keras_callbacks=[], optimizer=None):
        """:217-380.  -> (history, best_model_path); the final metrics of the best model are kept in self.metrics_trn /
        self.metrics_val (lists over the folds with val_type='cross_validate') and logged like the reference's."""
        dataset_paths, margin = check_fit_args(dataset_paths, shape, error_margin, batch, nb_epochs, val_type, prop_trn, prop_val,
                                               nb_folds, keras_callbacks, optimizer)
        shape = (int(tuple(shape)[0]),)
        logger = logging.getLogger('TrainableUNet1DSegmentation.fit')
        traces, spikes = [], []
        for p in dataset_paths:
            tr, sp = np.asarray(self.dataset_traces_func(p)), np.asarray(self.dataset_spikes_func(p))
            if tr.ndim != 2 or tr.shape != sp.shape:
                raise ValueError('%s: traces are %r and spikes %r; both must be the same (R,T) matrix' % (p, tr.shape, sp.shape))
            if tr.shape[1] < shape[0]:
                raise ValueError('%s: its traces are %d frames long, shorter than the window shape[0] = %d'
                                 % (p, tr.shape[1], shape[0]))
            traces += list(tr)
            spikes += list(sp)
        n = len(traces)
        if val_type == 'random_split':
            if int(n * prop_trn) < 1 or int(n * prop_val) < 1:
                raise ValueError('%d traces split %r / %r leave an empty training or validation set' % (n, prop_trn, prop_val))
            idxs_trn, idxs_val = split_random(n, prop_trn, prop_val)
            history, mt, mv, best = self._fit_single(traces, spikes, idxs_trn, idxs_val, shape, margin, batch, nb_epochs,
                                                     keras_callbacks, optimizer)
            self.metrics_trn, self.metrics_val = mt, mv
            for k in sorted(mt):
                logger.info('%-20s trn=%-9.4f val=%-9.4f' % (k, mt[k], mv[k]))
            logger.info('Best model path: %s' % best)
            return history, best
        if int(n / nb_folds) < 1:
            raise ValueError('%d traces cannot fill %d folds' % (n, nb_folds))
        folds = split_folds(n, nb_folds)
        histories, bests, self.metrics_trn, self.metrics_val = [], [], [], []
        for v in range(nb_folds):
            idxs_trn = [i for k, fold in enumerate(folds) if k != v for i in fold]
            idxs_val = list(folds[v])
            assert not set(idxs_trn) & set(idxs_val)
            logger.info('Cross validation fold = %d' % v)
            history, mt, mv, best = self._fit_single(traces, spikes, idxs_trn, idxs_val, shape, margin, batch, nb_epochs,
                                                     keras_callbacks, optimizer)
            histories.append(history)
            bests.append(best)
            self.metrics_trn.append(mt)
            self.metrics_val.append(mv)
            for k in sorted(mt):
                logger.info('%-20s trn=%-10.4f val=%-10.4f' % (k, mt[k], mv[k]))
        for k in sorted(self.metrics_trn[0]):
            a, b = [m[k] for m in self.metrics_trn], [m[k] for m in self.metrics_val]
            logger.info('%-20s trn=%-9.4f (%.4f) val=%-9.4f (%.4f)' % (k, np.mean(a), np.std(a), np.mean(b), np.std(b)))
        return histories, bests[int(np.argmax([m['F2'] for m in self.metrics_val]))]


def fit_spikes_device(dataset_paths, cpdir=None, net_builder_func=unet1d_train_hip, **fit_args):
    """One call: TrainableUNet1DSegmentation(cpdir).fit(dataset_paths, **fit_args) -> (history, best_model_path)."""
    import tempfile
    args = dict(shape=(4096,), error_margin=4., batch=20, nb_epochs=20, val_type='random_split', prop_trn=0.8, prop_val=0.2,
                nb_folds=5, keras_callbacks=[], optimizer=None)
    unknown = sorted(set(fit_args) - set(args))
    if unknown:
        raise ValueError('fit_spikes_device: unknown fit() arguments %r' % (unknown,))
    args.update(fit_args)
    check_fit_args(dataset_paths, **args)
    model = TrainableUNet1DSegmentation(cpdir if cpdir is not None else tempfile.mkdtemp(prefix='spikes_unet1d_'),
                                        net_builder_func=net_builder_func)
    return model.fit(dataset_paths, **args)
