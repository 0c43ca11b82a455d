"""Training the spikes model, the host side (deep_calcium_amd/spikes_fit.py, unet1d_train.py) without a GPU: argument checks,
the dataset reader, the label margin pooling, the sampler's RNG call sequence, the index splits and the metric formulas; and
the float64 training oracle of the GPU tests (tests/_unet1d_train_ref.py) against its own second opinion."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _unet1d_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES = ('dc_conv1d_stats', 'dc_conv1d_k5_wgrad', 'dc_conv1d_k5_c1_wgrad', 'dc_maxpool1d_2_bwd', 'dc_upsample1d_2x_drop_fwd',
            'dc_upsample1d_2x_drop_bwd', 'dc_spike_head_train_fwd', 'dc_spike_head_train_bwd')


def test_public_names_and_abi():
    import deep_calcium_amd
    from deep_calcium_amd import _build, _gen_tape, _lib, spikes, spikes_fit, unet1d_train
    assert deep_calcium_amd.TrainableUNet1DSegmentation is spikes_fit.TrainableUNet1DSegmentation
    assert deep_calcium_amd.fit_spikes_device is spikes_fit.fit_spikes_device
    assert deep_calcium_amd.get_dataset_spikes is spikes_fit.get_dataset_spikes
    assert deep_calcium_amd.UNet1DTrainEngine is unet1d_train.UNet1DTrainEngine
    assert {'TrainableUNet1DSegmentation', 'fit_spikes_device', 'get_dataset_spikes', 'UNet1DTrainEngine'} <= set(deep_calcium_amd.__all__)
    assert issubclass(spikes_fit.TrainableUNet1DSegmentation, spikes.UNet1DSegmentation)
    assert _lib.header_abi_version() >= 111 and 'spikes_train.hip' in _build.SOURCES
    protos = _lib.parse_header()
    tapeable = set(n for n, _ in _gen_tape.prototypes())
    for name in LAUNCHES:
        assert name in protos and name in tapeable, name
    for name in ('dc_conv1d_stats_blocks', 'dc_conv1d_k5_wgrad_ws_floats', 'dc_conv1d_k5_wgrad_blocks', 'dc_conv1d_k5_c1_wgrad_ws_floats',
                 'dc_spike_head_train_fwd_blocks', 'dc_spike_head_train_bwd_blocks'):
        assert name in protos, name
    header = open(_lib.HEADER).read()
    assert 'unet_1d_segmentation.py:49-148' in header and ':217-380' in header and 'utils/spikes.py:11-57' in header


def test_size_queries_run_without_gpu(dclib):
    L = dclib
    assert L.dc_conv1d_stats_blocks(1, 4) == 1 and L.dc_conv1d_stats_blocks(20 * 4096, 32) >= 64
    # the reference's 20 x 4096 batch, a 32 x 32 layer: the contraction is split so that the chip is filled
    parts = L.dc_conv1d_k5_wgrad_blocks(20, 4096, 32, 32)
    assert 256 <= parts <= 512
    assert L.dc_conv1d_k5_wgrad_ws_floats(20, 4096, 32, 32) == (parts + 32) * 5 * 32 * 32
    assert L.dc_conv1d_k5_wgrad_blocks(1, 1, 4, 4) == 1
    assert L.dc_conv1d_k5_wgrad_ws_floats(1, 16, 6, 4) == 0 and L.dc_conv1d_k5_wgrad_blocks(0, 16, 4, 4) == 0
    assert L.dc_conv1d_k5_c1_wgrad_ws_floats(20, 4096, 32) > 5 * 32
    assert L.dc_spike_head_train_fwd_blocks(3, 193) == 6 and L.dc_spike_head_train_bwd_blocks(3, 129) == 6


def test_c_abi_argument_validation_returns_codes(dclib):
    c = dclib.cdll
    P = 4096                     # any non-null, 16-byte aligned value: every call below must fail before a launch

    def rejected(rc, word):
        assert rc in (-1, -3) and word in c.dc_last_error().decode(), (rc, c.dc_last_error())

    rejected(c.dc_conv1d_stats(None, 8, P, 10, 8, None), 'null pointer')
    rejected(c.dc_conv1d_stats(P, 8, P, 0, 8, None), 'pixels=0')
    rejected(c.dc_conv1d_stats(P, 8, P, 10, 6, None), 'C=6')
    rejected(c.dc_conv1d_stats(P, 4, P, 10, 8, None), 'z_ld')
    rejected(c.dc_conv1d_k5_wgrad(P, P, P, None, 1, 8, 8, 8, None), 'null pointer')
    rejected(c.dc_conv1d_k5_wgrad(P, P + 4, P, P, 1, 8, 8, 8, None), 'aligned')
    rejected(c.dc_conv1d_k5_wgrad(P, P, P, P, 1, 0, 8, 8, None), 'T=0')
    rejected(c.dc_conv1d_k5_wgrad(P, P, P, P, 1, 8, 6, 8, None), 'Cin=6')
    rejected(c.dc_conv1d_k5_c1_wgrad(P, P, P, P, 1, 8, 6, None), 'Cout=6')
    rejected(c.dc_maxpool1d_2_bwd(P, None, 8, None, 0, P, 8, 1, 8, 8, None), 'null pointer')
    rejected(c.dc_maxpool1d_2_bwd(P, P, 4, None, 0, P, 8, 1, 8, 8, None), 'in_ld')
    rejected(c.dc_maxpool1d_2_bwd(P, P, 8, P, 4, P, 8, 1, 8, 8, None), 'skip_ld')
    rejected(c.dc_maxpool1d_2_bwd(P, P, 8, None, 0, P, 4, 1, 8, 8, None), 'dx_ld')
    rejected(c.dc_upsample1d_2x_drop_fwd(P, None, 8, None, 0.5, 1, 1, 8, 8, None), 'null pointer')
    rejected(c.dc_upsample1d_2x_drop_fwd(P, P, 8, None, 0.0, 1, 1, 8, 8, None), 'keep')
    rejected(c.dc_upsample1d_2x_drop_bwd(P, 4, None, 0.5, 1, P, 1, 8, 8, None), 'ld=4')
    rejected(c.dc_spike_head_train_fwd(P, P, P, 5, None, 2.0, 1.0, P, P, 1, 8, 8, None), 'null pointer')
    for pool in (0, 65):
        rejected(c.dc_spike_head_train_fwd(P, P, P, pool, P, 2.0, 1.0, P, P, 1, 8, 8, None), 'pool=%d' % pool)
        rejected(c.dc_spike_head_train_bwd(P, P, P, pool, P, 2.0, 1.0, P, P, 1, 8, 8, None), 'pool=%d' % pool)
    rejected(c.dc_spike_head_train_bwd(P, P, P, 5, P, 2.0, 1.0, P, P, 1, 8, 6, None), 'C=6')


def test_argument_errors_come_before_torch_or_the_library(tmp_path):
    code = r'''
import sys, numpy as np
from deep_calcium_amd import spikes_fit, unet1d_train
from deep_calcium_amd.traces import write_traces_dataset
d = sys.argv[1]
ds = write_traces_dataset(d + '/ds.hdf5', np.random.rand(3, 80), 'n', spikes=np.zeros((3, 80)))
short = write_traces_dataset(d + '/short.hdf5', np.random.rand(3, 40), 'short-one', spikes=np.zeros((3, 40)))
nosp = write_traces_dataset(d + '/nosp.hdf5', np.random.rand(3, 80), 'n')
m = spikes_fit.TrainableUNet1DSegmentation(d + '/cp')
def bad(f, *a, **k):
    word = k.pop('word', None)
    try:
        f(*a, **k)
    except ValueError as e:
        assert word is None or word in str(e), (word, str(e))
        return
    raise SystemExit('no ValueError: %r %r' % (a, k))
ok = dict(shape=(64,))
for f in (m.fit, spikes_fit.fit_spikes_device):
    bad(f, ds, **ok)
    bad(f, [], **ok)
    bad(f, [d + '/missing.hdf5'], **ok)
    for s in ((60,), (0,), (64, 64), 64, None, ('a',)):
        bad(f, [ds], shape=s)
    for e in (-1., 64., 'x', None):
        bad(f, [ds], error_margin=e, **ok)
    for b in (0, -1, 2.5, None, True):
        bad(f, [ds], batch=b, **ok)
        bad(f, [ds], nb_epochs=b, **ok)
    bad(f, [ds], val_type='holdout', **ok)
    bad(f, [ds], nb_folds=1, **ok)
    bad(f, [ds], prop_trn=0.8, prop_val=0.3, **ok)
    bad(f, [ds], prop_trn=1.0, prop_val=0.0, **ok)
    bad(f, [ds], keras_callbacks=[object()], **ok)
    bad(f, [ds], optimizer='adam', **ok)
bad(spikes_fit.fit_spikes_device, [ds], epochs=3)
bad(m.fit, [ds, short], word='short.hdf5', **ok)          # a trace shorter than the window: the dataset is named
bad(m.fit, [nosp], word='spikes', **ok)
E = unet1d_train.UNet1DTrainEngine
bad(E, (60,)); bad(E, (64, 64)); bad(E, (64,), nb_filters_base=6); bad(E, (64,), nb_filters_base=128)
bad(E, (64,), margin=64); bad(E, (64,), margin=-1); bad(E, (64,), prop_dropout_base=0.5)
bad(E, (64,), conv_kernel_init='orthogonal')
assert 'torch' not in sys.modules and 'deep_calcium_amd._lib' not in sys.modules, sorted(k for k in sys.modules if 'torch' in k)[:5]
print('ok')
'''
    out = subprocess.run([sys.executable, '-c', code, str(tmp_path)], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == 'ok', (out.stdout[-500:], out.stderr[-800:])


def test_base_class_fit_is_still_not_implemented(tmp_path):
    from deep_calcium_amd import spikes
    with pytest.raises(NotImplementedError):
        spikes.UNet1DSegmentation(str(tmp_path / 'cp')).fit([])


def test_get_dataset_spikes(tmp_path):
    from deep_calcium_amd import spikes_fit
    from deep_calcium_amd.traces import write_traces_dataset
    rs = np.random.RandomState(0)
    tr = rs.rand(4, 50).astype(np.float32)
    sp = (rs.uniform(size=(4, 50)) < 0.1).astype(np.uint8)
    for ext in ('hdf5', 'npz'):
        path = write_traces_dataset(str(tmp_path / ('ds.' + ext)), tr, 'experiment-001', spikes=sp)
        got = spikes_fit.get_dataset_spikes(path)
        assert got.dtype == np.uint8 and np.array_equal(got, sp), ext
        bare = write_traces_dataset(str(tmp_path / ('bare.' + ext)), tr, 'experiment-002')
        with pytest.raises(ValueError, match='spikes'):
            spikes_fit.get_dataset_spikes(bare)


@pytest.mark.parametrize('margin', [0, 1, 4, 4.7])
def test_label_margin_pooling_is_tensorflow_same(margin):
    from deep_calcium_amd.spikes_fit import pool_labels
    rs = np.random.RandomState(int(margin * 10))
    spikes = [(rs.uniform(size=T) < 0.1).astype(np.uint8) for T in (50, 50, 3, 1, 17)]        # 3 and 1: shorter than the pool
    got = pool_labels(spikes, margin)
    for s, g in zip(spikes, got):
        want = ref.pool_same(s.astype(np.float64)[None, :, None], int(margin) + 1)[0, :, 0]
        assert g.dtype == np.float32 and np.array_equal(g, want)
    if margin == 1:                                   # pool 2 looks at t and t + 1
        assert np.array_equal(pool_labels([np.array([0, 0, 1, 0, 0])], 1)[0], [0, 1, 1, 0, 0])


def test_sampler_draws_in_the_reference_order():
    """Per pass one choice(replace=False) over the traces, then one randint(0, len - T) per window, from numpy's global RNG."""
    from deep_calcium_amd.spikes_fit import batch_gen
    rs = np.random.RandomState(3)
    lens = [100, 70, 64, 91, 130]
    traces = [rs.randn(n) for n in lens]
    spikes = [(rs.uniform(size=n) < 0.2).astype(np.float32) for n in lens]
    T, batch, steps = 64, 3, 2
    np.random.seed(1234)
    gen = batch_gen(traces, spikes, (T,), batch, steps)
    got = [next(gen) for _ in range(2 * steps + 1)]                 # two passes and the first batch of a third
    np.random.seed(1234)
    k = 0
    for _pass in range(3):
        order = np.random.choice(np.arange(len(traces)), len(traces), replace=False)
        j = 0
        for _step in range(steps):
            if k == len(got):
                break
            tb, sb = got[k]
            assert tb.shape == (batch, T) and tb.dtype == np.float64 and sb.shape == (batch, T) and sb.dtype == np.uint8
            for b in range(batch):
                idx = order[j % len(order)]
                j += 1
                x0 = np.random.randint(0, lens[idx] - T) if lens[idx] > T else 0          # len == T: x0 = 0, nothing drawn
                assert np.array_equal(tb[b], traces[idx][x0:x0 + T]) and np.array_equal(sb[b], spikes[idx][x0:x0 + T]), (k, b)
            k += 1
    assert k == len(got)
    # a trace exactly T long alone: always the whole trace
    np.random.seed(0)
    tb, sb = next(batch_gen([traces[2]], [spikes[2]], (T,), 2, 1))
    assert np.array_equal(tb[0], traces[2]) and np.array_equal(tb[1], traces[2])


def test_index_splits():
    from deep_calcium_amd.spikes_fit import split_folds, split_random
    for n, pt, pv in ((12, 0.8, 0.2), (10, 0.75, 0.25), (7, 0.5, 0.5)):
        np.random.seed(n)
        trn, val = split_random(n, pt, pv)
        assert len(trn) == int(n * pt) and len(val) == int(n * pv)
        assert not set(trn) & set(val) and set(trn) | set(val) <= set(range(n))
        np.random.seed(n)
        idxs = np.random.choice(np.arange(n), n, replace=0)
        assert np.array_equal(trn, idxs[:int(n * pt)]) and np.array_equal(val, idxs[-int(n * pv):])
    for n, k in ((12, 2), (13, 5), (7, 3)):
        np.random.seed(n)
        folds = split_folds(n, k)
        assert len(folds) == k and all(len(f) == int(n / k) for f in folds)
        flat = [i for f in folds for i in f]
        assert len(set(flat)) == len(flat) and set(flat) <= set(range(n))


def test_metric_formulas_from_the_four_sums():
    import _unet1d_train_ref as tref
    from deep_calcium_amd.unet1d_train import metrics_from_sums
    rs = np.random.RandomState(5)
    B, T = 4, 50
    for case in range(3):
        p = rs.uniform(size=(B, T))
        y = (rs.uniform(size=(B, T)) < 0.2).astype(np.float64)
        if case == 1:
            p[0, :10] = 0.5                      # rounds to 0 (half to even)
            y[0, :10] = 1.
        if case == 2:
            p *= 0.4                             # nothing predicted: the epsilon keeps every quotient finite
        r = np.round(p)
        if case == 1:
            assert (r[0, :10] == 0).all()
        loss = tref.loss_np(p, y)
        sums = np.concatenate([[loss * B * T], tref.metric_sums(p, y)])
        got = metrics_from_sums(sums, B, T)
        tp, fn = (r * y).sum(), np.clip(y - r, 0, 1).sum()
        prec, reca = tp / (r.sum() + 1e-7), tp / (tp + fn + 1e-7)
        want = [loss, 5. * prec * reca / (4. * prec + reca + 1e-7), prec, reca, y.sum(1).mean(), r.sum(1).mean()]
        assert np.all(np.isfinite(got)) and np.allclose(got, want, rtol=1e-12, atol=1e-15), (case, got, want)
        if case == 2:
            assert got[1] == 0. and got[2] == 0. and got[3] == 0. and got[5] == 0.


def test_training_oracle_head_backward_has_a_second_opinion():
    import _unet1d_train_ref as tref
    rs = np.random.RandomState(2)
    for pool in (1, 2, 5, 64):
        for T in (1, 3, 40):
            a = np.maximum(rs.randn(2, T, 4), 0.)
            kh, bh = rs.randn(4, 2), rs.randn(2) * 0.1
            y = (rs.uniform(size=(2, T)) < 0.3).astype(np.uint8)
            loss, p, da, dkh, dbh = tref.head_loss_grads(a, kh, bh, pool, y)
            da2, dkh2, dbh2 = tref.head_bwd_np(a, kh, bh, pool, y)
            assert np.allclose(p, ref.head(a, kh, bh, pool), atol=1e-14) and abs(loss - tref.loss_np(p, y)) < 1e-12
            assert np.abs(da - da2).max() < 1e-12 and np.abs(dkh - dkh2).max() < 1e-12 and np.abs(dbh - dbh2).max() < 1e-12


def test_training_oracle_in_inference_statistics_limit_matches_the_inference_oracle():
    """The training graph with dropout off equals the inference oracle once the moving statistics ARE the batch statistics."""
    import _unet1d_train_ref as tref
    w = ref.make_model(4, 1, head_scale=1.0)
    x = ref.make_traces(3, 32, 2)
    y = np.zeros((3, 32), np.uint8)
    step = tref.TrainStep(w, 4, drp=0.).run(x, y, {})
    w2 = [np.array(a, np.float64) for a in w]
    for i, v in step.moving.items():                  # moving' = 0.99 moving + 0.01 batch  ->  batch
        w2[i] = (v - 0.99 * np.asarray(w[i], np.float64)) / 0.01
    assert np.abs(ref.forward(w2, x, 4) - step.p).max() < 1e-9
