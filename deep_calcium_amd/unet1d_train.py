"""UNet1D training engine: the reference's spikes network (models/spikes/unet_1d_segmentation.py:49-148) as its fit() trains it
(:217-380) -- batch statistics in BatchNormalization, Dropout active, the weighted loss and the metrics of utils/spikes.py:11-57,
Keras-form Adam --, on the dc_conv1d_* / dc_spike_head_train_* kernels of include/dcunet.h (UNet1D training section) and the
BatchNorm / ReLU / Dropout / Adam kernels the 2-D network already uses (a [N][T][C] activation is a [N*T][C] tensor).

    eng = UNet1DTrainEngine((4096,), nb_filters_base=32, margin=4)
    loss, F2, prec, reca, ytspks, ypspks = eng.train_on_batch(x, y)        # x float32 (B,T), y {0,1} (B,T); numpy or CUDA tensors
    eng.evaluate(x, y); eng.predict(x); eng.get_weights(); eng.set_weights(w); eng.save(path)

The 110 arrays of get_weights() live in one flat device buffer: the 74 trainable ones (kernel, bias, gamma, beta per conv_layer,
then the head's kernel and bias) first -- the range Adam steps over, with flat gradient / m / v buffers beside it --, the 36
moving statistics behind them; every array starts on a 16-byte boundary.  All activations of a step are kept for the backward.
A step is issued launch by launch from Python on torch's current stream; nothing synchronises until the metric sums are read.
Left out on purpose: launch tapes, data parallelism, the split-fp16 path.  evaluate() / predict() run in inference mode through
a UNet1DEngine that is rebuilt when the weights changed.

Importing this module needs neither torch nor the GPU; constructing an engine does (there is no CPU fallback).
"""
import numpy as np

from .unet1d import LEVELS, MAX_POOL, N_ARRAYS, conv_plan, expected_shapes

BN_EPS = 1e-3
BN_MOMENTUM = 0.99
K_EPS = 1e-7
METRIC_NAMES = ['loss', 'F2', 'prec', 'reca', 'ytspks', 'ypspks']
DROP_SITES = ('e1', 'e2', 'e3', 'u3', 'u2', 'u1', 'u0')


def drop_rates(drp):
    """Dropout rates: drp, 2drp, 2drp after encoder levels 1-3 (:96,:102,:108), 2drp, 2drp, 2drp, drp after the four up-samplings."""
    return {'e1': drp, 'e2': 2 * drp, 'e3': 2 * drp, 'u3': 2 * drp, 'u2': 2 * drp, 'u1': 2 * drp, 'u0': drp}


def drop_mask_shapes(nfb, B, T):
    """Shapes of the explicit uint8 {0,1} dropout masks train_on_batch(drop_masks=...) takes, by site."""
    s = {}
    for lvl in (1, 2, 3):
        s['e%d' % lvl] = (B, T >> lvl, nfb << lvl)
    for lvl in (3, 2, 1, 0):
        s['u%d' % lvl] = (B, T >> lvl, 2 * (nfb << lvl))
    return s


def metrics_from_sums(sums, windows, samples):
    """[loss, F2, prec, reca, ytspks, ypspks] (utils/spikes.py:30-57 as Keras averages them over a batch) from the head's sums
    {sum l, sum round(p) y, sum round(p), sum clip(y - round(p), 0, 1), sum y} over `windows` windows of `samples` samples."""
    ls, tp, spr, fn, sy = [float(v) for v in sums[:5]]
    prec = tp / (spr + K_EPS)
    reca = tp / (tp + fn + K_EPS)
    f2 = (1. + 2. ** 2) * ((prec * reca) / (2. ** 2 * prec + reca + K_EPS))
    return [ls / (float(windows) * samples), f2, prec, reca, sy / windows, spr / windows]


def check_train_args(window_shape, nb_filters_base, prop_dropout_base, margin):
    """Every argument error is a ValueError before torch or the library is touched.  -> (T, nfb, drp, margin)."""
    try:
        (T,) = tuple(window_shape)
        T, nfb, margin, drp = int(T), int(nb_filters_base), int(margin), float(prop_dropout_base)
    except (TypeError, ValueError):
        raise ValueError('window_shape must be a tuple of one integer, nb_filters_base and margin integers, prop_dropout_base a '
                         'number: got %r, %r, %r, %r' % (window_shape, nb_filters_base, margin, prop_dropout_base))
    if T < 16 or T % 16:
        raise ValueError('window_shape[0] must be a positive multiple of 16, not %d' % T)
    if nfb < 4 or nfb > 64 or nfb & (nfb - 1):
        raise ValueError('nb_filters_base must be a power of two in 4..64 for training (the BatchNorm kernels), not %d' % nfb)
    if not 0 <= margin < MAX_POOL:
        raise ValueError('margin must be in 0..%d, not %d' % (MAX_POOL - 1, margin))
    if not 0. <= drp < 0.5:
        raise ValueError('prop_dropout_base must be in [0, 0.5) (twice it is a dropout rate), not %r' % (drp,))
    return T, nfb, drp, margin


def initial_weights(nfb, conv_kernel_init='he_normal', seed=7535):
    """Keras-2.0.6 initialisers: he_normal (VarianceScaling(2, fan_in, normal truncated at 2 sigma), fan_in = 5 Cin) for the
    conv kernels -- or a callable shape -> array --, glorot_uniform (fan_in = nfb, fan_out = 2) for the head, zero biases,
    identity BatchNorm.  -> the 110 arrays."""
    rs = np.random.RandomState(seed)

    def he(shape):
        if callable(conv_kernel_init):
            return np.asarray(conv_kernel_init(shape), np.float32).reshape(shape)
        if conv_kernel_init != 'he_normal':
            raise ValueError('conv_kernel_init %r: he_normal or a callable shape -> array' % (conv_kernel_init,))
        out = rs.standard_normal(shape)
        bad = np.abs(out) > 2
        while bad.any():
            out[bad] = rs.standard_normal(int(bad.sum()))
            bad = np.abs(out) > 2
        return (out * np.sqrt(2. / (shape[0] * shape[1]))).astype(np.float32)

    w = []
    for cin, cout in conv_plan(nfb):
        w += [he((5, cin, cout)), np.zeros(cout, np.float32), np.ones(cout, np.float32), np.zeros(cout, np.float32),
              np.zeros(cout, np.float32), np.ones(cout, np.float32)]
    lim = np.sqrt(6. / (nfb + 2))
    return w + [rs.uniform(-lim, lim, (1, nfb, 2)).astype(np.float32), np.zeros(2, np.float32)]


class UNet1DTrainEngine(object):
    def __init__(self, window_shape, nb_filters_base=32, conv_kernel_init='he_normal', prop_dropout_base=0.05, margin=4,
                 device=None, seed=7535, weightpos=2., weightneg=1.):
        self.T, self.nfb, self.drp, self.margin = check_train_args(window_shape, nb_filters_base, prop_dropout_base, margin)
        self.window_shape = (self.T,)
        self.wpos, self.wneg = float(weightpos), float(weightneg)
        self.plan = conv_plan(self.nfb)
        weights = initial_weights(self.nfb, conv_kernel_init, seed)

        from ._reader import _open_device
        torch, _, self.L, self.device = _open_device(device, 'UNet1DTrainEngine')
        self._torch = torch

        # flat layout: trainable arrays first (Adam's range), the moving statistics behind; 16-byte aligned starts
        shapes = expected_shapes(self.nfb)
        self.shapes = shapes
        order = [i for i in range(N_ARRAYS) if i % 6 < 4 or i >= 108] + [i for i in range(108) if i % 6 >= 4]
        self.off, n = {}, 0
        for i in order:
            self.off[i] = n
            n += (int(np.prod(shapes[i])) + 3) // 4 * 4
            if i == N_ARRAYS - 1:
                self.n_train = n
        self.n_all = n
        mk = lambda k, dt=torch.float32: torch.zeros(k, dtype=dt, device=self.device)      # noqa: E731
        self.pflat, self.gflat, self.mflat, self.vflat = mk(self.n_all), mk(self.n_train), mk(self.n_train), mk(self.n_train)
        cmax = 16 * self.nfb
        self._ones, self._zeros = torch.ones(3 * cmax, dtype=torch.float32, device=self.device), mk(3 * cmax)
        self._bn = mk(2 * sum(co for _, co in self.plan))                 # mean | invstd of every conv_layer, this step
        self._wp_fwd = mk(sum(5 * ci * co for ci, co in self.plan[1:]))   # dc_pack_weights images, rebuilt every step
        self._wp_bwd = mk(sum(5 * ci * co for ci, co in self.plan[1:]))
        self._sums = torch.zeros(8, dtype=torch.float64, device=self.device)
        self.iterations = 0
        self.rng_seed = int(seed)
        self._B = 0
        self._infer = None
        self._version = 0
        self.optimizer = None
        self.set_weights(weights)

    # ---- parameters -------------------------------------------------------------------------------------------------
    def _p(self, i):
        return self.pflat.data_ptr() + 4 * self.off[i]

    def _g(self, i):
        return self.gflat.data_ptr() + 4 * self.off[i]

    def get_weights(self):
        flat = self.pflat.cpu().numpy()
        return [flat[self.off[i]:self.off[i] + int(np.prod(s))].reshape(s).copy() for i, s in enumerate(self.shapes)]

    def set_weights(self, weights):
        if len(weights) != N_ARRAYS:
            raise ValueError('a UNet1D model has %d weight arrays, got %d' % (N_ARRAYS, len(weights)))
        flat = np.zeros(self.n_all, np.float32)
        for i, (w, s) in enumerate(zip(weights, self.shapes)):
            if tuple(np.shape(w)) != s:
                raise ValueError('weight array %d has shape %r, the UNet1D graph (nb_filters_base %d) has %r there'
                                 % (i, tuple(np.shape(w)), self.nfb, s))
            flat[self.off[i]:self.off[i] + int(np.prod(s))] = np.asarray(w, np.float32).ravel()
        self.pflat.copy_(self._torch.from_numpy(flat))
        self._version += 1

    def grads(self):
        """The gradients of the last train step in get_weights() order (None for the moving statistics)."""
        flat = self.gflat.cpu().numpy()
        return [flat[self.off[i]:self.off[i] + int(np.prod(s))].reshape(s).copy() if (i % 6 < 4 or i >= 108) else None
                for i, s in enumerate(self.shapes)]

    def save(self, path):
        """A Keras 2.0.6 model file (keras_io.write_keras_unet1d) that UNet1DSegmentation.predict reads, `margin` included."""
        from .keras_io import write_keras_unet1d
        write_keras_unet1d(path, self.get_weights(), dict(nb_filters_base=self.nfb, window_shape=self.window_shape,
                                                          prop_dropout_base=self.drp, margin=self.margin))
        return path

    # ---- buffers ----------------------------------------------------------------------------------------------------
    def _buffers(self, B):
        if B == self._B:
            return
        torch, L, nfb, T = self._torch, self.L, self.nfb, self.T
        per = B * T * nfb
        mk = lambda k: torch.empty(max(int(k), 4), dtype=torch.float32, device=self.device)      # noqa: E731
        self._z = [mk(B * (T >> self._lvl(k)) * co) for k, (_, co) in enumerate(self.plan)]
        # activations: the second conv_layer of encoder levels 0-3 writes the skip slice of cat[lvl]; the others are dense
        self._cat = [mk(3 * per) for _ in range(LEVELS - 1)]
        self._dcat = [mk(3 * per) for _ in range(LEVELS - 1)]
        self._act = [None if (k % 2 == 1 and k < 8) else mk(B * (T >> self._lvl(k)) * co) for k, (_, co) in enumerate(self.plan)]
        self._pool = [None] + [mk(per >> 1) for _ in range(LEVELS - 1)]
        self._ga, self._gb, self._dz = mk(per), mk(per), mk(per)
        self._p_out = mk(B * T)
        part = ws = 8
        for k, (ci, co) in enumerate(self.plan):
            pixels = B * (T >> self._lvl(k))
            part = max(part, L.dc_bn_bwd_blocks(pixels, co) * co * 2)
            ws = max(ws, L.dc_conv1d_k5_c1_wgrad_ws_floats(B, T, co) if ci == 1 else
                     L.dc_conv1d_k5_wgrad_ws_floats(B, T >> self._lvl(k), ci, co))
        self._stat_part = torch.empty(max(L.dc_conv1d_stats_blocks(B * (T >> self._lvl(k)), co) * co * 2
                                          for k, (_, co) in enumerate(self.plan)), dtype=torch.float64, device=self.device)
        hb_f, hb_b = L.dc_spike_head_train_fwd_blocks(B, T), L.dc_spike_head_train_bwd_blocks(B, T)
        self._part = mk(max(part, hb_f * 8, hb_b * (2 * nfb + 2)))
        self._dbias_part = mk(part)
        self._ws = mk(max(ws, 32 * (2 * nfb + 2)))
        self._B = B

    @staticmethod
    def _lvl(k):
        return k // 2 if k < 10 else 3 - (k - 10) // 2

    def _act_ptr(self, k):
        """(pointer, sample stride) of conv_layer k's output activation."""
        co = self.plan[k][1]
        if k % 2 == 1 and k < 8:
            return self._cat[k // 2].data_ptr() + 4 * 2 * co, 3 * co
        return self._act[k].data_ptr(), co

    def _in_ptr(self, k, x_ptr):
        """Pointer of conv_layer k's (dense) input."""
        if k == 0:
            return x_ptr
        if k % 2 == 1:
            return self._act[k - 1].data_ptr()
        return self._pool[k // 2].data_ptr() if k < 10 else self._cat[self._lvl(k)].data_ptr()

    def _site_of_layer(self, k):
        return 'e%d' % (k // 2) if (k % 2 == 1 and 2 <= k < 8) else None

    def _drop_args(self, site, masks, step_seed):
        """(mask pointer or None, keep, seed) of a dropout site; keep 1 where the site has none."""
        if site is None:
            return None, 1.0, 0
        keep = 1.0 - drop_rates(self.drp)[site]
        if keep >= 1.0:
            return None, 1.0, 0
        if masks is not None:
            return masks[site].data_ptr(), keep, 0
        return None, keep, (step_seed * 16 + DROP_SITES.index(site)) & ((1 << 63) - 1)

    # ---- one train step ---------------------------------------------------------------------------------------------
    def _stage(self, x, y, drop_masks):
        torch = self._torch
        x = torch.as_tensor(np.ascontiguousarray(x, np.float32) if not isinstance(x, torch.Tensor) else x)
        y = torch.as_tensor(np.ascontiguousarray(y) if not isinstance(y, torch.Tensor) else y)
        if x.dim() != 2 or int(x.shape[1]) != self.T or int(x.shape[0]) < 1 or tuple(y.shape) != tuple(x.shape):
            raise ValueError('x and y must be (B >= 1, %d) matrices, not %r and %r' % (self.T, tuple(x.shape), tuple(y.shape)))
        x = x.to(self.device, torch.float32).contiguous()
        y = (y.to(self.device) > 0.5).to(torch.uint8).contiguous()
        masks = None
        if drop_masks is not None:
            shapes = drop_mask_shapes(self.nfb, int(x.shape[0]), self.T)
            masks = {}
            for site, shp in shapes.items():
                if 1.0 - drop_rates(self.drp)[site] >= 1.0:
                    continue
                m = drop_masks.get(site)
                if m is None or tuple(np.shape(m)) != shp:
                    raise ValueError('drop_masks[%r] must have shape %r' % (site, shp))
                masks[site] = torch.as_tensor(np.ascontiguousarray(m) if not isinstance(m, torch.Tensor) else m) \
                    .to(self.device, torch.uint8).contiguous()
        return x, y, masks

    def forward_backward(self, x, y, drop_masks=None):
        """Training-mode forward and backward of one batch: the gradients land in gflat, the BatchNorm moving statistics are
        updated, the head's sums are left on the device (read_sums()).  No parameter moves."""
        torch, L, nfb, T = self._torch, self.L, self.nfb, self.T
        x, y, masks = self._stage(x, y, drop_masks)
        B = int(x.shape[0])
        with torch.cuda.device(self.device):
            main = torch.cuda.current_stream(self.device)
            st = main.cuda_stream
            self._buffers(B)
            step_seed = self.rng_seed * 1000003 + self.iterations
            ones, zeros = self._ones.data_ptr(), self._zeros.data_ptr()
            xp, yp = x.data_ptr(), y.data_ptr()
            part, ws, dz = self._part.data_ptr(), self._ws.data_ptr(), self._dz.data_ptr()

            # the packed images of this step's kernels: forward form and flipped / transposed for the data gradient
            wpf, wpb, po = {}, {}, 0
            for k, (ci, co) in enumerate(self.plan):
                if ci == 1:
                    continue
                wpf[k] = self._wp_fwd.data_ptr() + 4 * po
                wpb[k] = self._wp_bwd.data_ptr() + 4 * po
                L.dc_pack_weights(self._p(6 * k), wpf[k], 5, ci, co, ci * co, co, 1, 0, st)
                L.dc_pack_weights(self._p(6 * k), wpb[k], 5, co, ci, ci * co, 1, co, 1, st)
                po += 5 * ci * co
            bn_off, o = {}, 0
            for k, (_, co) in enumerate(self.plan):
                bn_off[k] = (self._bn.data_ptr() + 4 * o, self._bn.data_ptr() + 4 * (o + co))
                o += 2 * co

            def conv_layer(k, t):
                ci, co = self.plan[k]
                i, pixels = 6 * k, B * t
                z = self._z[k].data_ptr()
                src = self._in_ptr(k, xp)
                if ci == 1:
                    L.dc_conv1d_k5_c1_fwd(src, self._p(i), ones, self._p(i + 1), 0, z, co, B, t, co, st)
                else:
                    L.dc_conv1d_k5_fwd(src, wpf[k], ones, self._p(i + 1), 0, z, co, B, t, ci, co, st)
                blocks = L.dc_conv1d_stats_blocks(pixels, co)
                L.dc_conv1d_stats(z, co, self._stat_part.data_ptr(), pixels, co, st)
                mean, invstd = bn_off[k]
                L.dc_bn_stats_finalize(self._stat_part.data_ptr(), blocks, 1, co, float(pixels), BN_EPS, BN_MOMENTUM, mean, invstd,
                                       self._p(i + 4), self._p(i + 5), st)
                mptr, keep, seed = self._drop_args(self._site_of_layer(k), masks, step_seed)
                out, ld = self._act_ptr(k)
                L.dc_bn_relu_drop_fwd(z, mean, invstd, self._p(i + 2), self._p(i + 3), mptr, keep, seed, out, ld, pixels, co,
                                      0.0, None, st)

            for lvl in range(LEVELS):
                c, t = nfb << lvl, T >> lvl
                if lvl:
                    L.dc_maxpool1d_2_fwd(self._cat[lvl - 1].data_ptr() + 4 * c, 3 * (c >> 1), self._pool[lvl].data_ptr(), B, 2 * t,
                                         c >> 1, st)
                conv_layer(2 * lvl, t)
                conv_layer(2 * lvl + 1, t)
            for j, lvl in enumerate((3, 2, 1, 0)):
                c, t = nfb << lvl, T >> lvl
                mptr, keep, seed = self._drop_args('u%d' % lvl, masks, step_seed)
                L.dc_upsample1d_2x_drop_fwd(self._act[9 + 2 * j].data_ptr(), self._cat[lvl].data_ptr(), 3 * c, mptr, keep, seed,
                                            B, t >> 1, 2 * c, st)
                conv_layer(10 + 2 * j, t)
                conv_layer(11 + 2 * j, t)
            a_head = self._act[17].data_ptr()
            pool = self.margin + 1
            L.dc_spike_head_train_fwd(a_head, self._p(108), self._p(109), pool, yp, self.wpos, self.wneg, self._p_out.data_ptr(),
                                      part, B, T, nfb, st)
            L.dc_reduce_partials_f64(part, L.dc_spike_head_train_fwd_blocks(B, T), 8, self._sums.data_ptr(), st)

            # ---- backward ----
            ga, gb = self._ga.data_ptr(), self._gb.data_ptr()
            L.dc_spike_head_train_bwd(a_head, self._p(108), self._p(109), pool, yp, self.wpos, self.wneg, ga, part, B, T, nfb, st)
            L.dc_reduce_partials(part, L.dc_spike_head_train_bwd_blocks(B, T), 2 * nfb + 2, 1.0, self._g(108), ws, st)

            def bwd_layer(k, t, da, da_ld, dx, dx_ld):
                """BatchNorm / ReLU / Dropout backward of conv_layer k, its bias / kernel gradients and (dx != None) its data
                gradient, written with sample stride dx_ld."""
                ci, co = self.plan[k]
                i, pixels = 6 * k, B * t
                z = self._z[k].data_ptr()
                mean, invstd = bn_off[k]
                gamma, beta = self._p(i + 2), self._p(i + 3)
                mptr, keep, seed = self._drop_args(self._site_of_layer(k), masks, step_seed)
                blocks = L.dc_bn_bwd_blocks(pixels, co)
                L.dc_bn_bwd_reduce(da, da_ld, z, mean, invstd, gamma, beta, mptr, keep, seed, part, None, pixels, co, st)
                L.dc_bn_bwd_finalize(part, blocks, co, self._g(i + 2), self._g(i + 3), st)
                L.dc_bn_bwd_apply(da, da_ld, z, mean, invstd, gamma, beta, mptr, keep, seed, self._g(i + 2), self._g(i + 3), dz,
                                  self._dbias_part.data_ptr(), None, pixels, co, st)
                L.dc_bn_bwd_apply_finalize(self._dbias_part.data_ptr(), None, blocks, co, 1024.0, self._g(i + 1), None, st)
                src = self._in_ptr(k, xp)
                if ci == 1:
                    L.dc_conv1d_k5_c1_wgrad(src, dz, self._g(i), ws, B, t, co, st)
                else:
                    L.dc_conv1d_k5_wgrad(src, dz, self._g(i), ws, B, t, ci, co, st)
                    if dx is not None:
                        L.dc_conv1d_k5_fwd(dz, wpb[k], ones, zeros, 0, dx, dx_ld, B, t, co, ci, st)

            for j, lvl in reversed(list(enumerate((3, 2, 1, 0)))):
                c, t = nfb << lvl, T >> lvl
                dcat = self._dcat[lvl].data_ptr()
                bwd_layer(11 + 2 * j, t, ga, c, gb, c)
                bwd_layer(10 + 2 * j, t, gb, c, dcat, 3 * c)
                mptr, keep, seed = self._drop_args('u%d' % lvl, masks, step_seed)
                L.dc_upsample1d_2x_drop_bwd(dcat, 3 * c, mptr, keep, seed, ga, B, t >> 1, 2 * c, st)
            for lvl in range(LEVELS - 1, -1, -1):
                c, t = nfb << lvl, T >> lvl
                if lvl < LEVELS - 1:
                    # ga: gradient of the pooled tensor; the skip gradient sits in channels [2C, 3C) of the decoder conv's dx
                    L.dc_maxpool1d_2_bwd(ga, self._cat[lvl].data_ptr() + 4 * 2 * c, 3 * c, self._dcat[lvl].data_ptr() + 4 * 2 * c,
                                         3 * c, gb, c, B, t, c, st)
                    ga, gb = gb, ga
                bwd_layer(2 * lvl + 1, t, ga, c, gb, c)
                bwd_layer(2 * lvl, t, gb, c, ga if lvl else None, c >> 1)
            x.record_stream(main)
            y.record_stream(main)
        self._version += 1                       # the moving statistics moved
        return self._p_out[:B * T].view(B, T)

    def read_sums(self):
        """The head's five sums of the last forward (synchronises)."""
        return self._sums.cpu().numpy()[:5]

    def adam_step(self, lr=0.002, beta_1=0.9, beta_2=0.999, epsilon=1e-8):
        """Keras-2.0.6 Adam over the trainable range; `iterations` counts completed steps."""
        torch = self._torch
        t = self.iterations + 1
        lr_t = float(lr * np.sqrt(1.0 - beta_2 ** t) / (1.0 - beta_1 ** t))
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream(self.device).cuda_stream
            self.L.dc_adam_step_flat(self.pflat.data_ptr(), self.gflat.data_ptr(), self.mflat.data_ptr(), self.vflat.data_ptr(),
                                     self.n_train, lr_t, beta_1, beta_2, epsilon, 1.0, st)
        self.iterations = t
        self._version += 1

    def compile(self, optimizer=None):
        """optimizer: an object with lr / beta_1 / beta_2 / epsilon (model.Adam); None = Adam(0.002), the reference's."""
        self.optimizer = optimizer

    def train_on_batch(self, x, y, drop_masks=None):
        """-> [loss, F2, prec, reca, ytspks, ypspks] of this batch in training mode, as Keras' train_on_batch reports them."""
        self.forward_backward(x, y, drop_masks)
        o = self.optimizer
        if o is None:
            self.adam_step(0.002)
        else:
            self.adam_step(float(o.lr), o.beta_1, o.beta_2, o.epsilon)
        return metrics_from_sums(self.read_sums(), self._B, self.T)

    # ---- inference mode ---------------------------------------------------------------------------------------------
    def _inference(self):
        if self._infer is None or self._infer[0] != self._version:
            from .unet1d import UNet1DEngine
            self._infer = (self._version, UNet1DEngine(self.get_weights(), self.nfb, self.margin, device=self.device))
        return self._infer[1]

    def predict(self, x, batch_size=32):
        """x (R,T) numpy -> float32 (R,T) probabilities in inference mode."""
        torch = self._torch
        eng = self._inference()
        xd = torch.as_tensor(np.ascontiguousarray(x, np.float32)).to(self.device)
        if xd.dim() != 2 or int(xd.shape[1]) % 16 or int(xd.shape[0]) < 1:
            raise ValueError('x must be (R >= 1, T) with T a multiple of 16, not %r' % (tuple(xd.shape),))
        outs = [eng.forward(xd[a:a + batch_size]) for a in range(0, int(xd.shape[0]), batch_size)]
        return torch.cat(outs, 0).cpu().numpy()

    def evaluate(self, x, y, batch_size=32):
        """-> [loss, F2, prec, reca, ytspks, ypspks] in inference mode, each the sample-weighted mean over the batches of
        `batch_size` (what Keras' evaluate reports)."""
        torch, L = self._torch, self.L
        eng = self._inference()
        x = np.ascontiguousarray(x, np.float32)
        y = np.ascontiguousarray(np.asarray(y) > 0.5, np.uint8)
        if x.ndim != 2 or x.shape != y.shape or x.shape[1] % 16 or x.shape[0] < 1:
            raise ValueError('x and y must be (R >= 1, T) matrices with T a multiple of 16, not %r and %r' % (x.shape, y.shape))
        R, T = x.shape
        xd, yd = torch.from_numpy(x).to(self.device), torch.from_numpy(y).to(self.device)
        total = np.zeros(6)
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream(self.device).cuda_stream
            for a in range(0, R, batch_size):
                xb, yb = xd[a:a + batch_size].contiguous(), yd[a:a + batch_size].contiguous()
                b = int(xb.shape[0])
                feats = eng.features(xb)
                blocks = L.dc_spike_head_train_fwd_blocks(b, T)
                part = torch.empty(blocks * 8, dtype=torch.float32, device=self.device)
                p = torch.empty((b, T), dtype=torch.float32, device=self.device)
                sums = torch.empty(8, dtype=torch.float64, device=self.device)
                L.dc_spike_head_train_fwd(feats, self._p(108), self._p(109), self.margin + 1, yb.data_ptr(), self.wpos, self.wneg,
                                          p.data_ptr(), part.data_ptr(), b, T, self.nfb, st)
                L.dc_reduce_partials_f64(part.data_ptr(), blocks, 8, sums.data_ptr(), st)
                total += b * np.asarray(metrics_from_sums(sums.cpu().numpy(), b, T))
        return list(total / R)
