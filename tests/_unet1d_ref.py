"""float64 reference of the spikes network for the tests: a plain numpy forward of unet1d (the reference's
models/spikes/unet_1d_segmentation.py:49-148) in inference mode, and a maker of random models.

Weights are the 110 arrays of Keras' get_weights(): per conv_layer kernel (5,Cin,Cout), bias, gamma, beta, moving_mean,
moving_variance; then the head's kernel (1,nfb,2) and bias (2,).  tests/test_spikes_api.py pins this forward against an
independent torch-CPU float64 one and guards the conditions that keep the random models informative."""
import numpy as np

EPS = 1e-3


def conv_plan(nfb):
    plan, cin = [], 1
    for lvl in range(5):
        c = nfb << lvl
        plan += [(cin, c), (c, c)]
        cin = c
    for lvl in (3, 2, 1, 0):
        c = nfb << lvl
        plan += [(3 * c, c), (c, c)]
    return plan


def make_model(nfb, seed, head_scale=0.07):
    """He-normal kernels, BatchNorm statistics near (but not at) the identity, a head scaled down so that the probabilities
    stay in mid range.  float32 arrays, get_weights() order."""
    rs = np.random.RandomState(seed)
    w = []
    for cin, cout in conv_plan(nfb):
        w.append(rs.randn(5, cin, cout) * np.sqrt(2. / (5 * cin)))
        w.append(rs.randn(cout) * 0.05)                       # bias
        w.append(1. + 0.1 * rs.randn(cout))                   # gamma
        w.append(0.1 * rs.randn(cout))                        # beta
        w.append(0.1 * rs.randn(cout))                        # moving_mean
        w.append(rs.uniform(0.5, 1.5, cout))                  # moving_variance
    w.append(rs.randn(1, nfb, 2) * np.sqrt(2. / nfb) * head_scale)
    w.append(rs.randn(2) * 0.05)
    return [a.astype(np.float32) for a in w]


def make_traces(R, T, seed):
    """z-scored traces as the network sees them: noise plus a few sharp transients, float32."""
    rs = np.random.RandomState(seed)
    x = rs.randn(R, T)
    for r in range(R):
        for t in rs.randint(0, T, size=max(1, T // 24)):
            x[r, t:t + 6] += 4. * np.exp(-np.arange(min(6, T - t)) / 2.)
    x = (x - x.mean(1, keepdims=True)) / np.maximum(x.std(1, keepdims=True), 1e-12) if T > 1 else x * 0
    return x.astype(np.float32)


def conv1d_k5(x, k):
    """x (N,T,Cin) float64, k (5,Cin,Cout): 'same', zero outside [0,T) of each trace."""
    N, T, _ = x.shape
    xp = np.pad(x, ((0, 0), (2, 2), (0, 0)))
    out = np.zeros((N, T, k.shape[2]))
    for tap in range(5):
        out += xp[:, tap:tap + T, :] @ k[tap]
    return out


def conv_layer(x, six, relu=True):
    k, b, ga, be, mm, mv = [np.asarray(a, np.float64) for a in six]
    z = conv1d_k5(x, k) + b
    y = (z - mm) / np.sqrt(mv + EPS) * ga + be
    return np.maximum(y, 0.) if relu else y


def maxpool2(x):
    N, T, C = x.shape
    return x[:, :T // 2 * 2].reshape(N, T // 2, 2, C).max(2)


def upsample2(x):
    return np.repeat(x, 2, axis=1)


def pool_same(l, pool):
    """MaxPooling1D(pool, strides=1, 'same') of l (N,T,J), TensorFlow's SAME: left pad (pool-1)//2, right pad pool//2, and
    the padding never wins (-inf)."""
    N, T, J = l.shape
    left, right = (pool - 1) // 2, pool // 2
    lp = np.pad(l, ((0, 0), (left, right), (0, 0)), constant_values=-np.inf)
    m = lp[:, 0:T]
    for k in range(1, pool):
        m = np.maximum(m, lp[:, k:k + T])
    return m


def head(a, kh, bh, pool):
    """a (N,T,C) -> p (N,T): logits, pooled, softmax channel -1."""
    l = a @ np.asarray(kh, np.float64).reshape(-1, 2) + np.asarray(bh, np.float64)
    m = pool_same(l, pool)
    return 1. / (1. + np.exp(m[..., 0] - m[..., 1]))


def features(weights, x):
    """x (R,T) with T % 16 == 0 -> the head's input (R,T,nfb), float64."""
    x = np.asarray(x, np.float64)[:, :, None]
    assert x.shape[1] % 16 == 0
    L = lambda i: weights[6 * i:6 * i + 6]      # noqa: E731
    skips, k = [], 0
    for lvl in range(5):
        if lvl:
            x = maxpool2(x)
        x = conv_layer(conv_layer(x, L(k)), L(k + 1))
        k += 2
        if lvl < 4:
            skips.append(x)
    for lvl in (3, 2, 1, 0):
        x = np.concatenate([upsample2(x), skips[lvl]], axis=-1)
        x = conv_layer(conv_layer(x, L(k)), L(k + 1))
        k += 2
    return x


def forward(weights, x, margin):
    """x (R,T) with T % 16 == 0 -> probabilities (R,T), float64."""
    return head(features(weights, x), weights[108], weights[109], margin + 1)


def forward_ragged(weights, x, margin):
    """Any T >= 1: the trace zero-extended on the right to the next multiple of 16, the output cropped (what predict() does)."""
    x = np.asarray(x, np.float64)
    R, T = x.shape
    xp = np.zeros((R, (T + 15) // 16 * 16))
    xp[:, :T] = x
    return forward(weights, xp, margin)[:, :T]


# (nfb, R, T, margin, model seed, trace seed) of the end-to-end GPU cases; test_spikes_api.py guards that each keeps the oracle
# informative (mid-range probabilities, both classes present, few samples at the threshold)
E2E_CASES = [
    (4, 5, 16, 4, 15, 1),
    (4, 3, 48, 1, 8, 2),
    (8, 4, 176, 4, 1, 3),
    (32, 3, 64, 0, 2, 4),
    (32, 2, 208, 4, 2, 5),
]
