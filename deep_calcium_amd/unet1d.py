"""UNet1D inference engine: the reference's spikes network (models/spikes/unet_1d_segmentation.py:49-148) as its predict() runs
it (:422-459), on the dc_conv1d_* / dc_spike_head_fwd kernels of include/dcunet.h.

    eng = UNet1DEngine(weights, nfb, margin)        # the 110 get_weights()-ordered arrays of keras_io.read_keras_unet1d
    p = eng.forward(x)                              # x: float32 (B, T) CUDA tensor, T % 16 == 0 -> float32 (B, T) probabilities

Inference only: Dropout is the identity, every BatchNormalization is folded once with its moving statistics (dc_bn_fold, eps
1e-3) into the (scale, shift) of the convolution in front of it.  A forward is 27 asynchronous launches on torch's current stream
(18 conv_layers, 4 poolings, 4 up-samplings, the head), issued from Python; nothing synchronises.  The skip tensors are written
straight into channels [2C, 3C) of the buffer the decoder's conv_layer reads, the up-sampled tensor into [0, 2C).

Importing this module needs neither torch nor the GPU; constructing a UNet1DEngine does (there is no CPU fallback).
"""
import numpy as np

LEVELS = 5
N_ARRAYS = 110
MAX_POOL = 64                        # dc_spike_head_fwd: pool = margin + 1 in 1..64


def conv_plan(nfb):
    """[(Cin, Cout)] of the 18 conv_layers in graph order (:89-137)."""
    plan, cin = [], 1
    for lvl in range(LEVELS):
        c = nfb << lvl
        plan += [(cin, c), (c, c)]
        cin = c
    for lvl in (3, 2, 1, 0):
        c = nfb << lvl
        plan += [(3 * c, c), (c, c)]
    return plan


def expected_shapes(nfb):
    """Shapes of the 110 arrays in get_weights() order."""
    out = []
    for cin, cout in conv_plan(nfb):
        out += [(5, cin, cout), (cout,), (cout,), (cout,), (cout,), (cout,)]
    return out + [(1, nfb, 2), (2,)]


def check_model(weights, nfb, margin):
    """Every argument error is a ValueError before the library or the GPU is touched.  -> (nfb, margin) as ints."""
    try:
        nfb, margin = int(nfb), int(margin)
    except (TypeError, ValueError):
        raise ValueError('nfb and margin must be integers, not %r and %r' % (nfb, margin))
    if nfb < 4 or nfb % 4:
        raise ValueError('nb_filters_base must be a positive multiple of 4, not %d' % nfb)
    if not 0 <= margin < MAX_POOL:
        raise ValueError('margin must be in 0..%d, not %d' % (MAX_POOL - 1, margin))
    if len(weights) != N_ARRAYS:
        raise ValueError('a UNet1D model has %d weight arrays, got %d' % (N_ARRAYS, len(weights)))
    for i, (w, shp) in enumerate(zip(weights, expected_shapes(nfb))):
        if tuple(np.shape(w)) != shp:
            raise ValueError('weight array %d has shape %r, the UNet1D graph (nb_filters_base %d) has %r there'
                             % (i, tuple(np.shape(w)), nfb, shp))
    return nfb, margin


class UNet1DEngine(object):
    def __init__(self, weights, nfb, margin, device=None):
        nfb, margin = check_model(weights, nfb, margin)
        self.nfb, self.margin = nfb, margin
        self.plan = conv_plan(nfb)

        from ._reader import _open_device
        torch, _, self.L, self.device = _open_device(device, 'UNet1DEngine')
        self._torch = torch

        # one flat upload; every array starts on a 16-byte boundary (the kernels read kernels / scale / shift as float4)
        offs, n = [], 0
        for w in weights:
            offs.append(n)
            n += (int(np.size(w)) + 3) // 4 * 4
        flat = np.zeros(n, np.float32)
        for w, o in zip(weights, offs):
            flat[o:o + np.size(w)] = np.asarray(w, np.float32).ravel()
        L = self.L
        with torch.cuda.device(self.device):
            st = torch.cuda.current_stream(self.device).cuda_stream
            self._raw = torch.from_numpy(flat).to(self.device)
            base = self._raw.data_ptr()
            ptr = lambda i: base + 4 * offs[i]                                     # noqa: E731
            self._packed = torch.empty(sum(5 * ci * co for ci, co in self.plan[1:]), dtype=torch.float32, device=self.device)
            self._affine = torch.empty(2 * sum(co for _, co in self.plan), dtype=torch.float32, device=self.device)
            self.layers = []           # (kernel pointer [packed; layer 0: plain], scale pointer, shift pointer, Cin, Cout)
            po = ao = 0
            for k, (ci, co) in enumerate(self.plan):
                i = 6 * k              # kernel, bias, gamma, beta, moving_mean, moving_variance
                if ci == 1:
                    wp = ptr(i)
                else:
                    wp = self._packed.data_ptr() + 4 * po
                    L.dc_pack_weights(ptr(i), wp, 5, ci, co, ci * co, co, 1, 0, st)
                    po += 5 * ci * co
                sc = self._affine.data_ptr() + 4 * ao
                sh = sc + 4 * co
                ao += 2 * co
                L.dc_bn_fold(ptr(i + 2), ptr(i + 3), ptr(i + 4), ptr(i + 5), ptr(i + 1), 1e-3, sc, sh, co, st)
                self.layers.append((wp, sc, sh, ci, co))
            self._kh, self._bh = ptr(N_ARRAYS - 2), ptr(N_ARRAYS - 1)
        self._cap = 0
        self._buf = {}

    def _buffers(self, B, T):
        """Owned by the engine, sized for the largest B * T seen: every level holds T_l * C_l = T * nfb floats per trace."""
        if B * T > self._cap:
            torch, per = self._torch, B * T * self.nfb
            self._buf = {}                                                 # release before allocating the larger set
            mk = lambda n: torch.empty(n, dtype=torch.float32, device=self.device)      # noqa: E731
            self._buf = dict(a=mk(per), b=mk(per), pool=mk(per // 2), cat=[mk(3 * per) for _ in range(LEVELS - 1)])
            self._cap = B * T
        return self._buf

    def forward(self, x):
        return self._run(x, True)

    def features(self, x):
        """Everything but the head: -> the device pointer of the head's input, dense float32 (B, T, nfb), in a buffer the
        engine owns (valid until its next call; ordered on torch's current stream).  The training engine's evaluate() puts
        dc_spike_head_train_fwd (the head plus loss and metric sums) on it."""
        return self._run(x, False)

    def _run(self, x, head):
        torch = self._torch
        if not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype != torch.float32:
            raise ValueError('x must be a float32 (B, T) tensor')
        if not x.is_cuda or x.device != self.device:
            raise ValueError('x is on %s, the engine on %s' % (x.device, self.device))
        B, T = int(x.shape[0]), int(x.shape[1])
        if B < 1 or T < 16 or T % 16:
            raise ValueError('x must be (B >= 1, T) with T a positive multiple of 16, not %r' % ((B, T),))
        x = x.contiguous()
        L, nfb = self.L, self.nfb
        with torch.cuda.device(self.device):
            main = torch.cuda.current_stream(self.device)
            st = main.cuda_stream
            buf = self._buffers(B, T)
            a, b, pool = buf['a'].data_ptr(), buf['b'].data_ptr(), buf['pool'].data_ptr()
            cat = [t.data_ptr() for t in buf['cat']]
            out = torch.empty((B, T), dtype=torch.float32, device=self.device) if head else None

            def conv(k, src, dst, ld, t):
                wp, sc, sh, ci, co = self.layers[k]
                if ci == 1:
                    L.dc_conv1d_k5_c1_fwd(src, wp, sc, sh, 1, dst, ld, B, t, co, st)
                else:
                    L.dc_conv1d_k5_fwd(src, wp, sc, sh, 1, dst, ld, B, t, ci, co, st)

            src = x.data_ptr()
            for lvl in range(LEVELS):
                c, t = nfb << lvl, T >> lvl
                if lvl:
                    L.dc_maxpool1d_2_fwd(cat[lvl - 1] + 4 * c, 3 * (c >> 1), pool, B, 2 * t, c >> 1, st)      # the skip slice below
                    src = pool
                conv(2 * lvl, src, a, c, t)
                if lvl < LEVELS - 1:
                    conv(2 * lvl + 1, a, cat[lvl] + 4 * 2 * c, 3 * c, t)            # skip: channels [2C, 3C) of the concat buffer
                else:
                    conv(2 * lvl + 1, a, b, c, t)
            for j, lvl in enumerate((3, 2, 1, 0)):
                c, t = nfb << lvl, T >> lvl
                L.dc_upsample1d_2x_fwd(b, cat[lvl], 3 * c, B, t >> 1, 2 * c, st)    # channels [0, 2C)
                conv(10 + 2 * j, cat[lvl], a, c, t)
                conv(11 + 2 * j, a, b, c, t)
            if head:
                L.dc_spike_head_fwd(b, self._kh, self._bh, self.margin + 1, out.data_ptr(), B, T, nfb, st)
            x.record_stream(main)
        return out if head else b
