"""UNet1D spike inference on the device (include/dcunet.h, UNet1D section; deep_calcium_amd/unet1d.py, spikes.py) against the
float64 oracle of tests/_unet1d_ref.py (pinned independently in test_spikes_api.py).

Tolerances.  Kernels: the project's parity contract, max |error| <= 1e-4 * max |reference| (expected: fp32 rounding of a K <= 3840
fmaf chain, ~1e-6).  Probabilities: 1e-4 absolute.  Pooling / up-sampling move values and are bit-exact.  Every test prints the
figure it asserts on."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

import _unet1d_ref as ref      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = -12345.5


def _st():
    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    return torch.from_numpy(np.array(a, order='C')).cuda()          # a copy: the shared fixtures are read-only


def _pack(dclib, k):
    """Keras (5,Cin,Cout) kernel -> the layout dc_conv1d_k5_fwd reads."""
    taps, cin, cout = k.shape
    src, dst = _dev(k), torch.empty(k.size, dtype=torch.float32, device='cuda')
    dclib.dc_pack_weights(src.data_ptr(), dst.data_ptr(), taps, cin, cout, cin * cout, cout, 1, 0, _st())
    return dst


def _conv_inputs(N, T, Cin, Cout, seed):
    rs = np.random.RandomState(seed)
    x = rs.randn(N, T, Cin).astype(np.float32)
    k = (rs.randn(5, Cin, Cout) * np.sqrt(2. / (5 * Cin))).astype(np.float32)
    scale = (1. + 0.2 * rs.randn(Cout)).astype(np.float32)
    shift = (0.3 * rs.randn(Cout)).astype(np.float32)
    return x, k, scale, shift


def _conv_ref(x, k, scale, shift, relu):
    y = ref.conv1d_k5(x.astype(np.float64), k.astype(np.float64)) * scale.astype(np.float64) + shift.astype(np.float64)
    return np.maximum(y, 0.) if relu else y


def _run_conv(dclib, x, k, scale, shift, relu, y_ld=None, chan0=0):
    N, T, Cin = x.shape
    Cout = k.shape[2]
    y_ld = y_ld or Cout
    y = torch.full((N, T, y_ld), POISON, dtype=torch.float32, device='cuda')
    xd, sc, sh = _dev(x), _dev(scale), _dev(shift)
    if Cin == 1:
        kd = _dev(k)
        dclib.dc_conv1d_k5_c1_fwd(xd.data_ptr(), kd.data_ptr(), sc.data_ptr(), sh.data_ptr(), int(relu), y.data_ptr() + 4 * chan0, y_ld,
                                  N, T, Cout, _st())
    else:
        kd = _pack(dclib, k)
        dclib.dc_conv1d_k5_fwd(xd.data_ptr(), kd.data_ptr(), sc.data_ptr(), sh.data_ptr(), int(relu), y.data_ptr() + 4 * chan0, y_ld,
                               N, T, Cin, Cout, _st())
    torch.cuda.synchronize()
    return y.cpu().numpy()


CONV_SHAPES = [(1, 1, 4, 4),           # all halo
               (2, 3, 8, 4),           # T shorter than the kernel
               (3, 37, 12, 36),        # ragged time tile, ragged column block, Cin = 3C
               (2, 130, 32, 32),       # one sample past a tile (and then two: 128 + 2)
               (2, 70, 768, 256),      # the widest K of the real network: 48 chunks
               (1, 260, 8, 72)]        # three time tiles (the last ragged), two column blocks (the second ragged), Cin below one chunk


@pytest.mark.parametrize('relu', [0, 1])
@pytest.mark.parametrize('shape', CONV_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_conv1d_k5_fwd(dclib, shape, relu):
    N, T, Cin, Cout = shape
    x, k, scale, shift = _conv_inputs(N, T, Cin, Cout, seed=N + T + Cin)
    want = _conv_ref(x, k, scale, shift, relu)
    got = _run_conv(dclib, x, k, scale, shift, relu)
    err = np.abs(got - want).max() / np.abs(want).max()
    print('dc_conv1d_k5_fwd %r relu=%d: max err / max |ref| = %.3g' % (shape, relu, err))
    assert err <= 1e-4


def test_conv1d_k5_fwd_writes_only_its_channel_slice(dclib):
    N, T, Cin, Cout = 3, 37, 12, 36
    x, k, scale, shift = _conv_inputs(N, T, Cin, Cout, seed=9)
    got = _run_conv(dclib, x, k, scale, shift, 1, y_ld=3 * Cout, chan0=2 * Cout)     # the skip slice of a concat buffer
    want = _conv_ref(x, k, scale, shift, 1)
    assert (got[..., :2 * Cout] == POISON).all()
    err = np.abs(got[..., 2 * Cout:] - want).max() / np.abs(want).max()
    print('dc_conv1d_k5_fwd into channels [2C, 3C): %.3g' % err)
    assert err <= 1e-4
    dense = _run_conv(dclib, x, k, scale, shift, 1)
    assert np.array_equal(dense, got[..., 2 * Cout:])


@pytest.mark.parametrize('shape', [(2, 3, 8, 4), (2, 130, 32, 32)], ids=lambda s: 'x'.join(map(str, s)))
def test_conv1d_k5_halo_never_crosses_traces(dclib, shape):
    """Trace 0 all zeros beside a large trace 1: trace 0's output must be the all-zero result, bit for bit (relu(shift))."""
    N, T, Cin, Cout = shape
    x, k, scale, shift = _conv_inputs(N, T, Cin, Cout, seed=4)
    x[0] = 0.
    x[1] = 1e6 * (1. + np.abs(x[1]))
    for relu in (0, 1):
        got = _run_conv(dclib, x, k, scale, shift, relu)
        zero = np.maximum(shift, 0.) if relu else shift
        assert np.array_equal(got[0], np.broadcast_to(zero, (T, Cout))), relu
        alone = _run_conv(dclib, x[1:], k, scale, shift, relu)
        assert np.array_equal(alone[0], got[1])


@pytest.mark.parametrize('shape', [(3, 1, 4), (2, 37, 32), (1, 130, 8)], ids=lambda s: 'x'.join(map(str, s)))
def test_conv1d_k5_c1_fwd(dclib, shape):
    N, T, Cout = shape
    x, k, scale, shift = _conv_inputs(N, T, 1, Cout, seed=T)
    for relu in (0, 1):
        want = _conv_ref(x, k, scale, shift, relu)
        got = _run_conv(dclib, x, k, scale, shift, relu, y_ld=Cout + 8, chan0=4)
        assert (got[..., :4] == POISON).all() and (got[..., 4 + Cout:] == POISON).all()
        err = np.abs(got[..., 4:4 + Cout] - want).max() / np.abs(want).max()
        print('dc_conv1d_k5_c1_fwd %r relu=%d: %.3g' % (shape, relu, err))
        assert err <= 1e-4
    x[0] = 0.                                   # the first trace's halo must not see the second
    x2 = np.concatenate([x[:1], 1e6 + 0 * x[:1]])
    got = _run_conv(dclib, x2, k, scale, shift, 0)
    assert np.array_equal(got[0], np.broadcast_to(shift, (T, Cout)))


@pytest.mark.parametrize('T', [1, 2, 7, 64])
def test_maxpool1d_2_fwd_is_bit_exact(dclib, T):
    N, C, ld = 3, 8, 24
    rs = np.random.RandomState(T)
    buf = rs.randn(N, T, ld).astype(np.float32)
    src = _dev(buf)
    out = torch.full((N, max(T // 2, 1), C), POISON, dtype=torch.float32, device='cuda')
    dclib.dc_maxpool1d_2_fwd(src.data_ptr() + 4 * 16, ld, out.data_ptr(), N, T, C, _st())      # the slice [16, 24) of a wider buffer
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    if T == 1:
        assert (got == POISON).all()            # documented: the output is empty, nothing is launched
        return
    want = ref.maxpool2(buf[..., 16:].astype(np.float64)).astype(np.float32)
    assert want.shape == (N, T // 2, C) and np.array_equal(got, want)


@pytest.mark.parametrize('T', [1, 5, 64])
def test_upsample1d_2x_fwd_is_bit_exact(dclib, T):
    N, C, ld = 2, 8, 12
    x = np.random.RandomState(T).randn(N, T, C).astype(np.float32)
    src = _dev(x)
    out = torch.full((N, 2 * T, ld), POISON, dtype=torch.float32, device='cuda')
    dclib.dc_upsample1d_2x_fwd(src.data_ptr(), out.data_ptr(), ld, N, T, C, _st())
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[..., :C], np.repeat(x, 2, axis=1)) and (got[..., C:] == POISON).all()


def _run_head(dclib, a, kh, bh, pool):
    N, T, C = a.shape
    ad, kd, bd = _dev(a), _dev(kh), _dev(bh)
    p = torch.full((N, T), POISON, dtype=torch.float32, device='cuda')
    dclib.dc_spike_head_fwd(ad.data_ptr(), kd.data_ptr(), bd.data_ptr(), pool, p.data_ptr(), N, T, C, _st())
    torch.cuda.synchronize()
    return p.cpu().numpy()


@pytest.mark.parametrize('C', [4, 32])
@pytest.mark.parametrize('pool', [1, 2, 5, 9, 64])
def test_spike_head_fwd(dclib, pool, C):
    worst = 0.
    for T in (1, 3, 64, 130, 200):               # 200: past the kernel's 192-sample tile, the window reaches across it
        rs = np.random.RandomState(pool * 1000 + T + C)
        a = np.maximum(rs.randn(2, T, C), 0.).astype(np.float32)
        kh = (rs.randn(C, 2) * np.sqrt(2. / C)).astype(np.float32)
        bh = (rs.randn(2) * 0.1).astype(np.float32)
        want = ref.head(a.astype(np.float64), kh, bh, pool)
        assert ((want > 0.05) & (want < 0.95)).mean() >= 0.5          # the oracle stays informative
        got = _run_head(dclib, a, kh, bh, pool)
        worst = max(worst, np.abs(got - want).max())
    print('dc_spike_head_fwd pool=%d C=%d: max |p - ref| = %.3g' % (pool, C, worst))
    assert worst <= 1e-4


@pytest.mark.parametrize('pool', [2, 4, 5])
def test_spike_head_pooling_side(dclib, pool):
    """One high logit at sample s raises exactly the samples whose window holds s: t in [s - pool/2, s + (pool-1)/2]."""
    T, C = 200, 4
    kh = np.zeros((C, 2), np.float32)
    kh[0, 1] = 1.                                # l1 = a[..., 0], l0 = 0
    bh = np.zeros(2, np.float32)
    for s in (0, 1, 100, 190, 191, 192, 193, T - 2, T - 1):
        a = np.zeros((1, T, C), np.float32)
        a[0, s, 0] = 10.
        got = _run_head(dclib, a, kh, bh, pool)[0]
        high = np.flatnonzero(got > 0.9)
        want = np.arange(max(0, s - pool // 2), min(T - 1, s + (pool - 1) // 2) + 1)
        assert np.array_equal(high, want), (pool, s, high)
        assert np.abs(np.delete(got, want) - 0.5).max() == 0.
        assert np.abs(got[want] - 1. / (1. + np.exp(-10.))).max() <= 1e-6


# ---- end to end -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(i):
    """(weights, traces, oracle probabilities) of E2E case i, computed once and shared (read only)."""
    nfb, R, T, margin, mseed, tseed = ref.E2E_CASES[i]
    w, x = ref.make_model(nfb, mseed), ref.make_traces(R, T, tseed)
    p = ref.forward(w, x, margin)
    for a in w + [x, p]:
        a.setflags(write=False)
    return w, x, p


@functools.lru_cache(maxsize=None)
def _engine(i):
    from deep_calcium_amd import UNet1DEngine
    nfb, R, T, margin, mseed, tseed = ref.E2E_CASES[i]
    return UNet1DEngine(_case(i)[0], nfb, margin)


@pytest.mark.parametrize('i', range(len(ref.E2E_CASES)), ids=lambda i: 'nfb%d-R%d-T%d-m%d' % ref.E2E_CASES[i][:4])
def test_engine_forward_equals_the_oracle(dclib, i):
    w, x, want = _case(i)
    got = _engine(i).forward(_dev(x))
    assert got.dtype == torch.float32 and got.is_cuda and tuple(got.shape) == x.shape
    err = np.abs(got.cpu().numpy() - want).max()
    print('UNet1DEngine.forward %r: max |p - oracle| = %.3g' % (ref.E2E_CASES[i][:4], err))
    assert err <= 1e-4


def test_engine_reuses_its_buffers_and_checks_its_input(dclib):
    eng = _engine(1)
    w, x, want = _case(1)
    big = eng.forward(_dev(np.concatenate([x, x, x])))                      # grows the buffers
    ptr = eng._buf['a'].data_ptr()
    small = eng.forward(_dev(x))
    assert eng._buf['a'].data_ptr() == ptr and torch.equal(big[:len(x)], small) and torch.equal(big[len(x):2 * len(x)], small)
    for bad in (_dev(x[:, :40]), _dev(x).double(), torch.from_numpy(np.array(x)), _dev(x)[0]):
        with pytest.raises(ValueError):
            eng.forward(bad)


def _write_case(tmp_path, i, name='experiment-001', ext='hdf5'):
    from deep_calcium_amd import keras_io
    from deep_calcium_amd.traces import write_traces_dataset
    nfb, R, T, margin, mseed, tseed = ref.E2E_CASES[i]
    w, x, p = _case(i)
    model_path = str(tmp_path / 'unet1d_model.hdf5')
    keras_io.write_keras_unet1d(model_path, w, dict(nb_filters_base=nfb, margin=margin))
    # raw traces whose z-score is (to float64 rounding) the oracle's input
    raw = 300. + 40. * x.astype(np.float64)
    ds = write_traces_dataset(str(tmp_path / ('traces.' + ext)), raw, name)
    return ds, model_path


@pytest.mark.parametrize('i,ext', [(2, 'hdf5'), (4, 'npz')])
def test_predict_equals_the_thresholded_oracle(dclib, tmp_path, i, ext):
    from deep_calcium_amd import UNet1DSegmentation
    from deep_calcium_amd.spikes import get_dataset_traces
    nfb, R, T, margin, mseed, tseed = ref.E2E_CASES[i]
    ds, model_path = _write_case(tmp_path, i, ext=ext)
    model = UNet1DSegmentation(str(tmp_path / 'cp'))
    spikes, names = model.predict([ds, ds], model_path, batch=3, threshold=0.5)
    assert names == ['experiment-001'] * 2 and len(spikes) == 2 and np.array_equal(spikes[0], spikes[1])
    s = spikes[0]
    assert s.dtype == np.uint8 and s.shape == (R, T) and set(np.unique(s)) <= {0, 1}
    want = ref.forward(_case(i)[0], get_dataset_traces(ds).astype(np.float32), margin)       # the oracle on what the device was given
    decided = np.abs(want - 0.5) > 1e-4
    print('predict %r: %.4f of the samples within 1e-4 of the threshold, %.3f positive' % (ref.E2E_CASES[i][:4], 1 - decided.mean(), s.mean()))
    assert 1 - decided.mean() <= 0.01
    assert np.array_equal(s[decided], (want > 0.5).astype(np.uint8)[decided])
    assert 0.05 <= s.mean() <= 0.95
    # another threshold moves the cut, not the probabilities
    thr = float(np.quantile(want, 0.9))
    s9 = model.predict([ds], model_path, threshold=thr)[0][0]
    far = np.abs(want - thr) > 1e-4
    assert np.array_equal(s9[far], (want > thr).astype(np.uint8)[far]) and s9.mean() < s.mean()


@pytest.mark.parametrize('T', [1, 17, 203])
def test_ragged_trace_lengths(dclib, tmp_path, T):
    from deep_calcium_amd import UNet1DSegmentation, keras_io
    nfb, margin = 4, 4
    w = ref.make_model(nfb, 15)
    model_path = str(tmp_path / 'm.hdf5')
    keras_io.write_keras_unet1d(model_path, w, dict(nb_filters_base=nfb, margin=margin))
    x = ref.make_traces(2, T, 20 + T)
    want = ref.forward_ragged(w, x, margin)
    got = UNet1DSegmentation(str(tmp_path / 'cp')).predict_proba(x, model_path)
    assert got.dtype == np.float32 and got.shape == (2, T)
    err = np.abs(got - want).max()
    print('ragged T=%d: max |p - oracle(zero-extended)| = %.3g' % (T, err))
    assert err <= 1e-4


def test_a_traces_probabilities_do_not_depend_on_the_batching(dclib, tmp_path):
    from deep_calcium_amd import UNet1DSegmentation, keras_io
    nfb, margin, R, T = 8, 4, 5, 176
    w = ref.make_model(nfb, 1)
    model_path = str(tmp_path / 'm.hdf5')
    keras_io.write_keras_unet1d(model_path, w, dict(nb_filters_base=nfb, margin=margin))
    x = ref.make_traces(R, T, 3)
    x[1] *= 1e3                                   # a neighbour that would show in any shared halo or shared scale
    model = UNet1DSegmentation(str(tmp_path / 'cp'))
    alone = np.concatenate([model.predict_proba(x[r:r + 1], model_path) for r in range(R)])
    b2 = model.predict_proba(x, model_path, batch=2)
    b32 = model.predict_proba(x, model_path, batch=32)
    rev = model.predict_proba(x[::-1], model_path, batch=3)[::-1]
    assert np.array_equal(alone, b2) and np.array_equal(alone, b32) and np.array_equal(alone, rev)
    assert model.model_reads == 1


def test_the_loaded_model_is_kept_while_its_file_is_unchanged(dclib, tmp_path):
    from deep_calcium_amd import UNet1DSegmentation, keras_io
    ds, model_path = _write_case(tmp_path, 1)
    nfb, R, T, margin, mseed, tseed = ref.E2E_CASES[1]
    model = UNet1DSegmentation(str(tmp_path / 'cp'))
    first = model.predict([ds], model_path)[0][0]
    assert model.model_reads == 1
    again = model.predict([ds], model_path)[0][0]
    assert model.model_reads == 1 and np.array_equal(first, again)
    w2 = [a.copy() for a in _case(1)[0]]
    w2[109] = np.array([3., -3.], np.float32)                # a head bias that votes "no spike" everywhere
    keras_io.write_keras_unet1d(model_path, w2, dict(nb_filters_base=nfb, margin=margin))
    st = os.stat(model_path)
    os.utime(model_path, ns=(st.st_atime_ns, st.st_mtime_ns + 1000000))
    third = model.predict([ds], model_path)[0][0]
    assert model.model_reads == 2 and third.sum() == 0 and first.sum() > 0


def test_example_command_writes_predicts_spikes(dclib, tmp_path):
    from deep_calcium_amd import UNet1DSegmentation, hdf5_min
    ds, model_path = _write_case(tmp_path, 1, name='nf.test')
    cp = str(tmp_path / 'cp')
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'spikes', 'unet1d.py'), 'predict', ds, '--model', model_path,
                          '-c', cp], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    f = hdf5_min.File(os.path.join(cp, 'nf.test_spikes.hdf5'))
    want = UNet1DSegmentation(cp).predict([ds], model_path)[0][0]
    got = f['spikes'].read()
    assert got.dtype == np.uint8 and np.array_equal(got, want) and want.sum() > 0
    assert np.array_equal(f['traces'].read(), hdf5_min.File(ds)['traces'].read())


def test_predict_spikes_device(dclib, tmp_path):
    from deep_calcium_amd import predict_spikes_device
    ds, model_path = _write_case(tmp_path, 1)
    w, x, want = _case(1)
    p = predict_spikes_device(x, model_path, proba=True)
    assert np.abs(p - want).max() <= 1e-4
    s = predict_spikes_device(ds, model_path, cpdir=str(tmp_path / 'cp'))
    assert s.dtype == np.uint8 and s.shape == x.shape
