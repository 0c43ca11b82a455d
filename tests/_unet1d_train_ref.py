"""float64 reference of the spikes network IN TRAINING for the tests, on top of _unet1d_ref.py: the training-mode graph of
unet1d (the reference's models/spikes/unet_1d_segmentation.py:49-148: batch statistics in BatchNormalization, Dropout active),
the weighted loss and the metrics of utils/spikes.py:11-57, and the backward pass by torch CPU float64 autograd.

    max_pool1d on the CPU routes the gradient to the FIRST maximum; the head's TensorFlow-'SAME' window is built with explicit
    -inf padding, the smaller pad on the left (so padding never wins).  head_bwd_np is a hand-written numpy float64 backward of
    the head's routing, a second opinion on the part most easily got wrong.

Dropout masks are explicit {0,1} arrays: 'e1','e2','e3' after encoder levels 1-3 (N, T >> lvl, nfb << lvl) and 'u3','u2','u1','u0'
on the up-sampled tensor entering decoder level lvl (N, T >> lvl, 2 * (nfb << lvl)); rates drp, 2drp, 2drp and 2drp, 2drp, 2drp, drp."""
import numpy as np
import torch
import torch.nn.functional as F

import _unet1d_ref as ref

EPS = ref.EPS
MOMENTUM = 0.99
K_EPS = 1e-7            # keras.backend.epsilon()


def t64(a):
    return torch.from_numpy(np.asarray(a, np.float64).copy())


def conv1d_k5_t(x, k):
    """x (N,T,Cin), k Keras (5,Cin,Cout): 'same', zero outside [0,T) of each trace.  torch tensors, float64."""
    return F.conv1d(x.permute(0, 2, 1), k.permute(2, 1, 0), padding=2).permute(0, 2, 1)


def conv_grads(x, k, dz):
    """(dx, dw) of z = conv1d_k5(x, k) for an upstream gradient dz, by autograd."""
    xt, kt = t64(x).requires_grad_(True), t64(k).requires_grad_(True)
    conv1d_k5_t(xt, kt).backward(t64(dz))
    return xt.grad.numpy(), kt.grad.numpy()


def pool_same_t(l, pool):
    """MaxPooling1D(pool, strides=1, 'same') of l (N,T,J): TensorFlow's SAME with explicit -inf padding."""
    left, right = (pool - 1) // 2, pool // 2
    lp = F.pad(l.permute(0, 2, 1), (left, right), value=float('-inf'))
    return F.max_pool1d(lp, pool, stride=1).permute(0, 2, 1)


def head_t(a, kh, bh, pool):
    m = pool_same_t(a @ kh.reshape(-1, 2) + bh, pool)
    return torch.sigmoid(m[..., 1] - m[..., 0]), m


def loss_t(p, y, wpos=2., wneg=1.):
    return (-(wpos * y * torch.log(p + 1e-7) + wneg * (1. - y) * torch.log(1. - p + 1e-7))).mean()


def head_loss_grads(a, kh, bh, pool, y, wpos=2., wneg=1.):
    """-> loss, p, da, dkh (C,2), dbh (2,) of the mean weighted loss, by autograd."""
    at, kt, bt = t64(a).requires_grad_(True), t64(kh).reshape(-1, 2).requires_grad_(True), t64(bh).requires_grad_(True)
    p, _ = head_t(at, kt, bt, pool)
    loss = loss_t(p, t64(y), wpos, wneg)
    loss.backward()
    return float(loss.detach()), p.detach().numpy(), at.grad.numpy(), kt.grad.numpy(), bt.grad.numpy()


def head_bwd_np(a, kh, bh, pool, y, wpos=2., wneg=1.):
    """The same gradients by hand: plain loops, first maximum of the clipped window."""
    a, kh, bh, y = np.asarray(a, np.float64), np.asarray(kh, np.float64).reshape(-1, 2), np.asarray(bh, np.float64), np.asarray(y, np.float64)
    N, T, C = a.shape
    left, right = (pool - 1) // 2, pool // 2
    l = a @ kh + bh
    dl = np.zeros_like(l)
    for n in range(N):
        for t in range(T):
            lo, hi = max(0, t - left), min(T - 1, t + right)
            arg = [lo + int(np.argmax(l[n, lo:hi + 1, j])) for j in (0, 1)]          # np.argmax: the first maximum
            d = l[n, arg[0], 0] - l[n, arg[1], 1]
            p, q = 1. / (1. + np.exp(d)), 1. / (1. + np.exp(-d))
            dldp = -wpos / (p + 1e-7) if y[n, t] else wneg / (1. - p + 1e-7)
            dm1 = dldp * p * q / (N * T)
            dl[n, arg[0], 0] -= dm1
            dl[n, arg[1], 1] += dm1
    return dl @ kh.T, np.einsum('ntc,ntj->cj', a, dl), dl.sum((0, 1))


def metric_sums(p, y):
    """{sum round(p) y, sum round(p), sum clip(y - round(p), 0, 1), sum y}; np.round is half to even like K.round."""
    p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
    r = np.round(p)
    return np.array([(r * y).sum(), r.sum(), np.clip(y - r, 0., 1.).sum(), y.sum()])


def loss_np(p, y, wpos=2., wneg=1.):
    p, y = np.asarray(p, np.float64), np.asarray(y, np.float64)
    return float((-(wpos * y * np.log(p + 1e-7) + wneg * (1. - y) * np.log(1. - p + 1e-7))).mean())


def pool2_bwd(x, dy):
    """Gradient of MaxPooling1D(2, strides=2) of x (N,T,C) for dy (N,T//2,C): torch CPU max_pool1d, first maximum."""
    xt = t64(x).requires_grad_(True)
    if x.shape[1] < 2:
        return np.zeros_like(np.asarray(x, np.float64))
    F.max_pool1d(xt.permute(0, 2, 1), 2, stride=2).permute(0, 2, 1).backward(t64(dy))
    return xt.grad.numpy()


def drop_rates(drp):
    return {'e1': drp, 'e2': 2 * drp, 'e3': 2 * drp, 'u3': 2 * drp, 'u2': 2 * drp, 'u1': 2 * drp, 'u0': drp}


def mask_shapes(nfb, N, T):
    s = {}
    for lvl in (1, 2, 3):
        s['e%d' % lvl] = (N, T >> lvl, nfb << lvl)
    for lvl in (3, 2, 1, 0):
        s['u%d' % lvl] = (N, T >> lvl, 2 * (nfb << lvl))
    return s


def make_masks(nfb, N, T, drp, seed):
    rs = np.random.RandomState(seed)
    rates = drop_rates(drp)
    return {k: (rs.uniform(size=shp) >= rates[k]).astype(np.uint8) for k, shp in mask_shapes(nfb, N, T).items()}


class TrainStep(object):
    """One training-mode forward + backward of the 110-array model in float64.  After run():
    loss, p (N,T), grads (list of 110, None for the moving statistics), moving (the updated moving statistics by array index),
    and margins = (min |pre-ReLU value|, min gap between two positive pool candidates, min head-window runner-up gap)."""

    def __init__(self, weights, margin, drp=0.05, wpos=2., wneg=1.):
        self.w = [t64(a).requires_grad_(i % 6 < 4 or i >= 108) for i, a in enumerate(weights)]
        self.margin, self.drp, self.wpos, self.wneg = margin, drp, wpos, wneg

    def _conv_layer(self, x, i):
        k, b, ga, be, mm, mv = self.w[6 * i:6 * i + 6]
        z = conv1d_k5_t(x, k) + b
        mu, var = z.mean((0, 1)), z.var((0, 1), unbiased=False)
        self.moving[6 * i + 4] = (mm * MOMENTUM + mu * (1. - MOMENTUM)).detach().numpy()
        self.moving[6 * i + 5] = (mv * MOMENTUM + var * (1. - MOMENTUM)).detach().numpy()
        yv = (z - mu) / torch.sqrt(var + EPS) * ga + be
        self.min_prerelu = min(self.min_prerelu, float(yv.detach().abs().min()))
        return torch.relu(yv)

    def _pool(self, x):
        a, b = x.detach()[:, 0::2], x.detach()[:, 1::2]
        both = (a > 0) | (b > 0)                     # two zeros tie exactly, on the device too: the first wins in both
        if both.any():
            self.min_poolgap = min(self.min_poolgap, float((a - b).abs()[both].min()))
        return F.max_pool1d(x.permute(0, 2, 1), 2, stride=2).permute(0, 2, 1)

    def _drop(self, x, key, masks):
        keep = 1. - drop_rates(self.drp)[key]
        return x if keep >= 1. else x * t64(masks[key]) / keep

    def run(self, x, y, masks):
        self.moving, self.min_prerelu, self.min_poolgap = {}, np.inf, np.inf
        h = t64(x)[:, :, None]
        skips, i = [], 0
        for lvl in range(5):
            if lvl:
                h = self._pool(h)
            h = self._conv_layer(self._conv_layer(h, i), i + 1)
            i += 2
            if 1 <= lvl <= 3:
                h = self._drop(h, 'e%d' % lvl, masks)
            if lvl < 4:
                skips.append(h)
        for lvl in (3, 2, 1, 0):
            h = self._drop(h.repeat_interleave(2, dim=1), 'u%d' % lvl, masks)
            h = torch.cat([h, skips[lvl]], dim=-1)
            h = self._conv_layer(self._conv_layer(h, i), i + 1)
            i += 2
        pool = self.margin + 1
        p, m = head_t(h, self.w[108], self.w[109], pool)
        # runner-up gap of every head window: the largest logit strictly below the window's maximum
        l = (h @ self.w[108].reshape(-1, 2) + self.w[109]).detach()
        left, right = (pool - 1) // 2, pool // 2
        lp = F.pad(l.permute(0, 2, 1), (left, right), value=float('-inf')).unfold(2, pool, 1)      # (N,2,T,pool)
        top = lp.topk(min(2, pool), dim=-1).values
        self.min_headgap = float((top[..., 0] - top[..., 1]).min()) if pool > 1 else np.inf
        loss = loss_t(p, t64(y), self.wpos, self.wneg)
        loss.backward()
        self.loss, self.p = float(loss.detach()), p.detach().numpy()
        self.grads = [None if w.grad is None else w.grad.numpy() for w in self.w]
        self.margins = (self.min_prerelu, self.min_poolgap, self.min_headgap)
        return self


def adam_keras(p, g, m, v, it, lr=0.002, b1=0.9, b2=0.999, eps=1e-8):
    """Keras 2.0.6 Adam, float64: `it` updates already done.  -> (p, m, v)."""
    t = it + 1
    lr_t = lr * np.sqrt(1. - b2 ** t) / (1. - b1 ** t)
    m = b1 * m + (1. - b1) * g
    v = b2 * v + (1. - b2) * g * g
    return p - lr_t * m / (np.sqrt(v) + eps), m, v
