#!/usr/bin/env python
"""Spike prediction with the HIP UNet1D path: what follows `examples/neurons/unet2ds_nf.py traces ...` on the same GPU.

    python examples/spikes/unet1d.py train a_traces.hdf5,b_traces.hdf5 [-c checkpoints_dir] [--epochs 20] [--shape 4096]
    python examples/spikes/unet1d.py predict neurofinder.00.00_traces.hdf5 --model unet1d_model.hdf5 [-c checkpoints_dir]

Reads dataset files of the spikes model's schema (models/spikes/unet_1d_segmentation.py:182-187: attribute `name`, `traces`
(no. ROIs, no. frames); what write_traces_dataset makes, .hdf5 or .npz) and a Keras model file of unet1d (:49-148), runs
UNet1DSegmentation.predict (:422-459) and writes `<checkpoints_dir>/<name>_spikes.hdf5`: the traces as they were read plus
`spikes`, the uint8 segmentation.  `train` needs `spikes` beside `traces` in its dataset files, runs
TrainableUNet1DSegmentation.fit (:217-380), prints the best model's path and writes it to `<checkpoints_dir>/best_model.txt`:
what `predict --model` takes.
"""
import argparse
import logging
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))

from deep_calcium_amd import UNet1DSegmentation, write_traces_dataset      # noqa: E402
from deep_calcium_amd.nf_datasets import default_dirs                      # noqa: E402
from deep_calcium_amd.spikes import _open_members                          # noqa: E402

CHECKPOINTS_DIR = '%s/spikes_unet1d' % default_dirs()[1]

logging.basicConfig(level=logging.INFO)


def training(dataset_paths, checkpoints_dir, shape=4096, error_margin=4., batch=20, epochs=20, val_type='random_split', nb_folds=5,
             nb_filters_base=32, prop_dropout_base=0.05, seed=None):
    from deep_calcium_amd.spikes_fit import TrainableUNet1DSegmentation, unet1d_train_hip
    logger = logging.getLogger('training')
    if seed is not None:
        np.random.seed(seed)

    def builder(window_shape, margin=4):
        return unet1d_train_hip(window_shape, margin=margin, nb_filters_base=nb_filters_base, prop_dropout_base=prop_dropout_base)

    model = TrainableUNet1DSegmentation(cpdir=checkpoints_dir, net_builder_func=builder)
    _, best = model.fit(dataset_paths.split(','), shape=(shape,), error_margin=error_margin, batch=batch, nb_epochs=epochs,
                        val_type=val_type, nb_folds=nb_folds)
    with open('%s/best_model.txt' % model.cpdir, 'w') as fp:
        fp.write(best + '\n')
    logger.info('best model: %s' % best)
    print(best)
    return best


def prediction(dataset_paths, model_path, checkpoints_dir, batch=32, threshold=0.5):
    logger = logging.getLogger('prediction')
    paths = dataset_paths.split(',')
    model = UNet1DSegmentation(cpdir=checkpoints_dir)
    spikes, names = model.predict(paths, model_path=model_path, batch=batch, threshold=threshold)
    outs = []
    for p, s, name in zip(paths, spikes, names):
        f = _open_members(p)[1]
        tr = f['traces']
        tr = np.array(tr.read() if hasattr(tr, 'read') else tr)
        f.close()
        out = write_traces_dataset('%s/%s_spikes.hdf5' % (model.cpdir, name), tr, name, spikes=s)
        logger.info('%s: %d traces of %d frames, %d spike samples -> %s' % (name, s.shape[0], s.shape[1], int(s.sum()), out))
        outs.append(out)
    return outs


if __name__ == '__main__':
    ap = argparse.ArgumentParser(description='CLI for the UNet1D spikes model.')
    sp = ap.add_subparsers(title='actions', description='Choose an action.')
    sp_trn = sp.add_parser('train', help='CLI for training.')
    sp_trn.set_defaults(which='train')
    sp_trn.add_argument('dataset_paths', help='dataset file(s) with traces and spikes, comma separated', type=str)
    sp_trn.add_argument('-c', '--checkpoints_dir', help='checkpoint directory', default=CHECKPOINTS_DIR)
    sp_trn.add_argument('--shape', help='window length (a multiple of 16)', default=4096, type=int)
    sp_trn.add_argument('--error_margin', help='frames within which a predicted spike counts', default=4., type=float)
    sp_trn.add_argument('--batch', help='windows per step', default=20, type=int)
    sp_trn.add_argument('--epochs', help='epochs', default=20, type=int)
    sp_trn.add_argument('--val_type', choices=['random_split', 'cross_validate'], default='random_split')
    sp_trn.add_argument('--nb_folds', default=5, type=int)
    sp_trn.add_argument('--nb_filters_base', default=32, type=int)
    sp_trn.add_argument('--prop_dropout_base', default=0.05, type=float)
    sp_trn.add_argument('--seed', help='seed of the sampler (numpy global RNG)', default=None, type=int)
    sp_prd = sp.add_parser('predict', help='CLI for prediction.')
    sp_prd.set_defaults(which='predict')
    sp_prd.add_argument('dataset_paths', help='traces dataset file(s), comma separated', type=str)
    sp_prd.add_argument('-m', '--model_path', '--model', help='path to model', required=True)
    sp_prd.add_argument('-c', '--checkpoints_dir', help='checkpoint directory', default=CHECKPOINTS_DIR)
    sp_prd.add_argument('--batch', help='traces per forward', default=32, type=int)
    sp_prd.add_argument('--threshold', help='prediction threshold', default=0.5, type=float)
    args = vars(ap.parse_args())
    if 'which' not in args:
        ap.error('choose an action: train, predict')
    if args.pop('which') == 'train':
        training(**args)
    else:
        prediction(**args)
