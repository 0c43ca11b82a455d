"""Spike inference without a GPU: the float64 oracle of the GPU tests pinned against an independent torch forward, the conditions
that keep its random models informative, the Keras file round trip, the host side of UNet1DSegmentation and the argument
checks of the new C ABI entry points (include/dcunet.h, UNet1D section)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _unet1d_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHES = ('dc_conv1d_k5_fwd', 'dc_conv1d_k5_c1_fwd', 'dc_maxpool1d_2_fwd', 'dc_upsample1d_2x_fwd', 'dc_spike_head_fwd')


def test_public_names_and_abi():
    import deep_calcium_amd
    from deep_calcium_amd import _gen_tape, _lib, spikes, unet1d
    assert deep_calcium_amd.UNet1DSegmentation is spikes.UNet1DSegmentation
    assert deep_calcium_amd.predict_spikes_device is spikes.predict_spikes_device
    assert deep_calcium_amd.UNet1DEngine is unet1d.UNet1DEngine
    assert {'UNet1DSegmentation', 'UNet1DEngine', 'predict_spikes_device'} <= set(deep_calcium_amd.__all__)
    assert _lib.header_abi_version() >= 110
    protos = _lib.parse_header()
    tapeable = set(n for n, _ in _gen_tape.prototypes())
    for name in LAUNCHES:
        assert name in protos and name in tapeable, name
    header = open(_lib.HEADER).read()
    assert 'unet_1d_segmentation.py:49-148' in header and 'unet_1d_segmentation.py:422-459' in header
    for cite in (':81-84', ':93', ':79', ':139-145'):
        assert cite in header, cite
    from deep_calcium_amd import _build
    assert 'spikes.hip' in _build.SOURCES


def test_modules_import_without_torch_or_the_library():
    code = ("import sys, deep_calcium_amd.spikes, deep_calcium_amd.unet1d; "
            "assert 'torch' not in sys.modules and 'deep_calcium_amd._lib' not in sys.modules; print('ok')")
    out = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == 'ok', out.stderr[-500:]


# ---- the oracle, pinned independently --------------------------------------------------------------------------------------
def _torch_forward(weights, x, margin):
    """unet1d in torch-CPU float64, channels-first, from torch's own conv / batch-norm / pooling.  The head's pooling is torch's
    symmetric max_pool1d: equal to TensorFlow 'SAME' only when margin is even (pool odd)."""
    torch = pytest.importorskip('torch')
    F = torch.nn.functional
    W = [torch.from_numpy(np.asarray(a, np.float64)) for a in weights]

    def conv_layer(h, i):
        k, b, ga, be, mm, mv = W[6 * i:6 * i + 6]
        h = F.conv1d(h, k.permute(2, 1, 0).contiguous(), b, padding=2)
        return F.relu(F.batch_norm(h, mm, mv, ga, be, training=False, eps=1e-3))

    h = torch.from_numpy(np.asarray(x, np.float64))[:, None, :]
    skips, k = [], 0
    for lvl in range(5):
        if lvl:
            h = F.max_pool1d(h, 2, 2)
        h = conv_layer(conv_layer(h, k), k + 1)
        k += 2
        if lvl < 4:
            skips.append(h)
    for lvl in (3, 2, 1, 0):
        h = torch.cat([h.repeat_interleave(2, dim=2), skips[lvl]], dim=1)
        h = conv_layer(conv_layer(h, k), k + 1)
        k += 2
    l = F.conv1d(h, W[108].permute(2, 1, 0).contiguous(), W[109])
    assert margin % 2 == 0
    l = F.max_pool1d(l, margin + 1, 1, padding=margin // 2)
    return torch.softmax(l, dim=1)[:, -1, :].numpy()


@pytest.mark.parametrize('nfb,R,T', [(4, 5, 16), (4, 3, 48), (8, 4, 176), (32, 2, 208)])
def test_oracle_equals_an_independent_torch_forward(nfb, R, T):
    w = ref.make_model(nfb, 3)
    x = ref.make_traces(R, T, 11)
    got, want = ref.forward(w, x, 4), _torch_forward(w, x, 4)
    err = np.abs(got - want).max()
    print('oracle vs torch float64: %.3g' % err)
    assert got.shape == (R, T) and err <= 1e-12


def _pool_loop(l, pool):
    """The pooling formula of include/dcunet.h, sample by sample."""
    N, T, J = l.shape
    m = np.empty_like(l)
    for n in range(N):
        for t in range(T):
            lo, hi = max(0, t - (pool - 1) // 2), min(T - 1, t + pool // 2)
            for j in range(J):
                m[n, t, j] = max(l[n, u, j] for u in range(lo, hi + 1))
    return m


@pytest.mark.parametrize('margin', [0, 1, 3, 4, 8])
@pytest.mark.parametrize('T', [1, 3, 16, 37])
def test_oracle_pooling_is_the_asymmetric_same_formula(margin, T):
    l = np.random.RandomState(5 * T + margin).randn(2, T, 2)
    assert np.array_equal(ref.pool_same(l, margin + 1), _pool_loop(l, margin + 1))
    if margin == 1 and T >= 3:          # pool 2 looks at t and t + 1, never at t - 1
        l = np.zeros((1, T, 2))
        l[0, 1] = 5.
        m = ref.pool_same(l, 2)
        assert m[0, 0, 0] == 5. and m[0, 1, 0] == 5. and m[0, 2, 0] == 0.


@pytest.mark.parametrize('margin', [1, 0])
def test_oracle_head_at_margins_torch_cannot_express(margin):
    """pool 2 (asymmetric: t and t + 1) and pool 1 (the identity): the oracle's head against the per-sample loop."""
    w = ref.make_model(4, 8)
    x = ref.make_traces(3, 48, 2)
    l = ref.features(w, x) @ np.asarray(w[108], np.float64).reshape(-1, 2) + np.asarray(w[109], np.float64)
    m = _pool_loop(l, margin + 1)
    want = np.exp(m[..., 1]) / (np.exp(m[..., 0]) + np.exp(m[..., 1]))          # softmax, channel -1
    assert np.abs(ref.forward(w, x, margin) - want).max() <= 1e-12
    if margin == 0:
        assert np.array_equal(m, l)


# ---- the fixtures of the GPU tests keep the oracle informative -------------------------------------------------------------
@pytest.mark.parametrize('case', ref.E2E_CASES, ids=lambda c: 'nfb%d-R%d-T%d-m%d' % c[:4])
def test_fixture_models_keep_the_oracle_informative(case):
    nfb, R, T, margin, mseed, tseed = case
    p = ref.forward(ref.make_model(nfb, mseed), ref.make_traces(R, T, tseed), margin)
    mid = np.mean((p >= 0.05) & (p <= 0.95))
    pos = np.mean(p > 0.5)
    near = np.mean(np.abs(p - 0.5) <= 1e-4)
    print('mid %.3f  positives %.3f  near threshold %.4f  range %.3f..%.3f' % (mid, pos, near, p.min(), p.max()))
    assert mid >= 0.5
    assert pos >= 0.05 and 1. - pos >= 0.05
    assert near <= 0.01
    assert p.max() - p.min() > 0.02                     # not a dead ReLU stack (exactly 0.5 everywhere)


# ---- keras_io ---------------------------------------------------------------------------------------------------------------
def test_keras_unet1d_round_trip(tmp_path):
    from deep_calcium_amd import hdf5_min, keras_io
    w = ref.make_model(4, 1)
    assert len(w) == 110 == keras_io.UNET1D_ARRAYS
    path = str(tmp_path / 'unet1d.hdf5')
    keras_io.write_keras_unet1d(path, w, dict(nb_filters_base=4, margin=2, window_shape=(4096,), prop_dropout_base=0.05))
    m = keras_io.read_keras_unet1d(path)
    assert len(m['weights']) == 110 and all(np.array_equal(a, b) and a.dtype == np.float32 for a, b in zip(m['weights'], w))
    assert m['config']['nb_filters_base'] == 4 and m['config']['margin'] == 2
    assert m['config']['window_shape'] == (4096,) and m['config']['prop_dropout_base'] == 0.05
    assert keras_io.read_keras_unet1d(path, margin=7)['config']['margin'] == 2          # the file's model_config wins
    f = hdf5_min.File(path)
    assert np.array_equal(f['model_weights/conv1d_1/conv1d_1/kernel:0'].read(), w[0])
    assert f['model_weights/batch_normalization_18/batch_normalization_18/moving_variance:0'].read().shape == (4,)
    assert f['model_weights/conv1d_19/conv1d_19/kernel:0'].read().shape == (1, 4, 2)
    names = [n.decode() for n in f['model_weights'].attrs['layer_names']]
    assert 'max_pooling1d_5' in names and 'up_sampling1d_4' in names and names[0] == 'input_1'


def test_weights_only_file_takes_the_callers_margin(tmp_path):
    from deep_calcium_amd import keras_io
    w = ref.make_model(4, 1)
    path = str(tmp_path / 'weights.hdf5')
    keras_io.write_keras_unet1d(path, w, dict(nb_filters_base=4, margin=2), weights_only=True)
    assert keras_io.read_keras_unet1d(path)['config']['margin'] == 4                   # the reference's error_margin
    assert keras_io.read_keras_unet1d(path, margin=1)['config']['margin'] == 1
    assert all(np.array_equal(a, b) for a, b in zip(keras_io.read_keras_unet1d(path)['weights'], w))


def test_each_reader_refuses_the_other_models_file(tmp_path):
    from deep_calcium_amd import keras_io
    p1 = str(tmp_path / 'unet1d.hdf5')
    keras_io.write_keras_unet1d(p1, ref.make_model(4, 1), dict(nb_filters_base=4))
    with pytest.raises(ValueError, match='UNet1D'):
        keras_io.read_keras_model(p1)
    # the UpSampling2D variant of UNet2DS also has 110 arrays: told apart by the first kernel's rank
    seq = keras_io.keras_layer_sequence(4, 0.25, True, (32, 32))
    w2 = [np.zeros(shp, np.float32) for *_, ws in seq for _, shp in ws]
    assert len(w2) == 110
    p2 = str(tmp_path / 'unet2ds.hdf5')
    keras_io.write_keras_model(p2, w2, dict(nb_filters_base=4, window_shape=(32, 32), upsampling_or_transpose='upsampling'))
    with pytest.raises(ValueError, match='UNet2DS'):
        keras_io.read_keras_unet1d(p2)
    assert len(keras_io.read_keras_model(p2)['weights']) == 110


def test_a_wrong_kernel_shape_names_the_layer(tmp_path, monkeypatch):
    from deep_calcium_amd import keras_io
    good = keras_io.unet1d_layer_sequence

    def bad(*a, **k):
        seq = good(*a, **k)
        i = [n for n, *_ in seq].index('conv1d_7')
        n, cls, cfg, ws = seq[i]
        seq[i] = (n, cls, cfg, [('kernel:0', (3,) + ws[0][1][1:]), ws[1]])
        return seq
    w = ref.make_model(4, 1)
    w[6 * 6] = w[6 * 6][:3]                                   # conv1d_7's kernel with 3 taps
    path = str(tmp_path / 'bad.hdf5')
    monkeypatch.setattr(keras_io, 'unet1d_layer_sequence', bad)
    keras_io.write_keras_unet1d(path, w, dict(nb_filters_base=4))
    monkeypatch.setattr(keras_io, 'unet1d_layer_sequence', good)
    with pytest.raises(ValueError, match='conv1d_7'):
        keras_io.read_keras_unet1d(path)
    with pytest.raises(ValueError, match='expected 110'):
        keras_io.write_keras_unet1d(path, w[:-1], dict(nb_filters_base=4))


# ---- UNet1DSegmentation on the host -----------------------------------------------------------------------------------------
def test_default_dataset_functions(tmp_path):
    from deep_calcium_amd import spikes
    from deep_calcium_amd.traces import write_traces_dataset
    rs = np.random.RandomState(0)
    tr = (rs.rand(4, 50) * 1000 + 200).astype(np.float32)
    tr[2] = 7.                                                # constant in time
    want = np.zeros((4, 50))
    ok = [0, 1, 3]
    t64 = tr.astype(np.float64)
    want[ok] = (t64[ok] - np.mean(t64[ok], axis=1, keepdims=True)) / np.std(t64[ok], axis=1, keepdims=True)
    for ext in ('hdf5', 'npz'):
        path = write_traces_dataset(str(tmp_path / ('ds.' + ext)), tr, 'experiment-001')
        got = spikes.get_dataset_traces(path)
        assert got.dtype == np.float64 and np.array_equal(got, want), ext
        assert (got[2] == 0).all()
        assert spikes.get_dataset_attrs(path)['name'] == 'experiment-001'
    model = spikes.UNet1DSegmentation(str(tmp_path / 'cp'))
    assert os.path.isdir(model.cpdir) and model.dataset_traces_func is spikes.get_dataset_traces
    with pytest.raises(NotImplementedError, match='training'):
        model.fit([str(tmp_path / 'ds.hdf5')])


def test_argument_errors_come_before_torch_or_the_library(tmp_path):
    code = r'''
import sys, numpy as np
from deep_calcium_amd import spikes, unet1d
from deep_calcium_amd.traces import write_traces_dataset
ds = write_traces_dataset(sys.argv[1] + '/ds.hdf5', np.random.rand(3, 20), 'n')
open(sys.argv[1] + '/model.hdf5', 'wb').close()
m = spikes.UNet1DSegmentation(sys.argv[1] + '/cp')
tr = np.zeros((3, 20))
def bad(f, *a, **k):
    try:
        f(*a, **k)
    except ValueError:
        return
    raise SystemExit('no ValueError: %r %r' % (a, k))
mp = sys.argv[1] + '/model.hdf5'
for b in (0, -1, 2.5, None, True):
    bad(m.predict, [ds], mp, batch=b)
    bad(m.predict_proba, tr, mp, batch=b)
    bad(spikes.predict_spikes_device, tr, mp, batch=b)
for t in (-0.1, 1.5, 'x', None):
    bad(m.predict, [ds], mp, threshold=t)
bad(m.predict, ds, mp)
bad(m.predict, [ds], sys.argv[1] + '/missing.hdf5')
bad(m.predict, [sys.argv[1] + '/missing.hdf5'], mp)
for x in (np.zeros(5), np.zeros((2, 3, 4)), np.zeros((0, 5)), np.zeros((2, 0)), np.array([['a']]), np.full((2, 4), np.nan)):
    bad(m.predict_proba, x, mp)
w = [np.zeros(s, np.float32) for s in unet1d.expected_shapes(4)]
bad(unet1d.UNet1DEngine, w, 6, 4)
bad(unet1d.UNet1DEngine, w, 4, 64)
bad(unet1d.UNet1DEngine, w, 4, -1)
bad(unet1d.UNet1DEngine, w[:-1], 4, 4)
bad(unet1d.UNet1DEngine, w, 8, 4)
assert 'torch' not in sys.modules and 'deep_calcium_amd._lib' not in sys.modules, sorted(k for k in sys.modules if 'torch' in k)[:5]
print('ok')
'''
    out = subprocess.run([sys.executable, '-c', code, str(tmp_path)], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == 'ok', (out.stdout[-500:], out.stderr[-800:])


# ---- C ABI ------------------------------------------------------------------------------------------------------------------
def test_c_abi_argument_validation_returns_codes(dclib):
    c = dclib.cdll
    P = 4096                     # any non-null, 16-byte aligned value: every call below must fail before a launch

    def rejected(rc, word):
        msg = c.dc_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    rejected(c.dc_conv1d_k5_fwd(None, P, P, P, 1, P, 8, 1, 8, 8, 8, None), 'null pointer')
    rejected(c.dc_conv1d_k5_fwd(P, P, P, P, 1, None, 8, 1, 8, 8, 8, None), 'null pointer')
    rejected(c.dc_conv1d_k5_fwd(P, P, P, P, 1, P, 8, 1, 8, 6, 8, None), 'Cin=6')
    rejected(c.dc_conv1d_k5_fwd(P, P, P, P, 1, P, 8, 1, 0, 8, 8, None), 'T=0')
    rejected(c.dc_conv1d_k5_fwd(P, P, P, P, 1, P, 8, 0, 8, 8, 8, None), 'N=0')
    rejected(c.dc_conv1d_k5_fwd(P, P, P, P, 1, P, 8, 1, 8, 8, 6, None), 'Cout=6')
    rejected(c.dc_conv1d_k5_fwd(P, P, P, P, 1, P, 4, 1, 8, 8, 8, None), 'y_ld')
    rejected(c.dc_conv1d_k5_fwd(P + 4, P, P, P, 1, P, 8, 1, 8, 8, 8, None), 'aligned')
    rejected(c.dc_conv1d_k5_c1_fwd(None, P, P, P, 1, P, 8, 1, 8, 8, None), 'null pointer')
    rejected(c.dc_conv1d_k5_c1_fwd(P, P, None, P, 1, P, 8, 1, 8, 8, None), 'null pointer')
    rejected(c.dc_conv1d_k5_c1_fwd(P, P, P, P, 1, P, 8, 1, 0, 8, None), 'T=0')
    rejected(c.dc_conv1d_k5_c1_fwd(P, P, P, P, 1, P, 8, 1, 8, 7, None), 'Cout=7')
    rejected(c.dc_maxpool1d_2_fwd(None, 8, P, 1, 8, 8, None), 'null pointer')
    rejected(c.dc_maxpool1d_2_fwd(P, 8, P, 1, 0, 8, None), 'T=0')
    rejected(c.dc_maxpool1d_2_fwd(P, 8, P, 1, 8, 6, None), 'C=6')
    rejected(c.dc_maxpool1d_2_fwd(P, 4, P, 1, 8, 8, None), 'in_ld')
    rejected(c.dc_upsample1d_2x_fwd(P, None, 8, 1, 8, 8, None), 'null pointer')
    rejected(c.dc_upsample1d_2x_fwd(P, P, 8, 1, 0, 8, None), 'T=0')
    rejected(c.dc_upsample1d_2x_fwd(P, P, 8, 1, 8, 2, None), 'C=2')
    rejected(c.dc_upsample1d_2x_fwd(P, P, 4, 1, 8, 8, None), 'out_ld')
    rejected(c.dc_spike_head_fwd(P, P, None, 5, P, 1, 8, 8, None), 'null pointer')
    rejected(c.dc_spike_head_fwd(P, P, P, 5, P, 1, 0, 8, None), 'T=0')
    rejected(c.dc_spike_head_fwd(P, P, P, 5, P, 1, 8, 6, None), 'C=6')
    for pool in (0, -1, 65):
        rejected(c.dc_spike_head_fwd(P, P, P, pool, P, 1, 8, 8, None), 'pool=%d' % pool)
