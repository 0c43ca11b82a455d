"""What every stage on an (R, T) matrix shares: the checks of the matrix, the device, the resident input and result().

A matrix stage (dff.TraceBaseline, merge.TracePairCorr, dynamics.TraceDynamics, deconv.TraceDeconvolver) takes a matrix of one row
per ROI or trace, numpy or already on the device, and returns results per row.  _MatrixStage holds everything about that which does
not depend on what the stage computes; a subclass adds its own argument checks, its kernels, its kinds and result_device().

Importing this module needs neither torch nor the GPU.
"""
import numpy as np


def _is_device_tensor(x):
    return not isinstance(x, np.ndarray) and hasattr(x, 'is_cuda') and hasattr(x, 'data_ptr')


def _check_matrix(x, what, dtypes, shape=None):
    """(R, T) of one of `dtypes` (numpy's names), numpy or a device tensor with contiguous rows, not empty and, if given, of
    `shape` -> (R, T); ValueError otherwise."""
    names = ' or '.join(dtypes)
    if _is_device_tensor(x):
        if not x.is_cuda or str(x.dtype) not in ['torch.' + d for d in dtypes] or x.dim() != 2:
            raise ValueError('%s must be an (R, T) %s tensor on the device, not %s %r' % (what, names, x.dtype, tuple(x.shape)))
        if x.shape[1] > 1 and x.stride(1) != 1 or x.shape[0] > 1 and x.stride(0) < x.shape[1]:
            raise ValueError('%s: the rows of a device tensor must be contiguous (strides %r)' % (what, tuple(x.stride())))
    elif isinstance(x, np.ndarray):
        if x.ndim != 2 or x.dtype.name not in dtypes:
            raise ValueError('%s must be an (R, T) %s array, not %s %r' % (what, names, x.dtype, x.shape))
    else:
        raise ValueError('%s must be a numpy array or a device tensor, not %s' % (what, type(x).__name__))
    got = (int(x.shape[0]), int(x.shape[1]))
    if got[0] < 1 or got[1] < 1:
        raise ValueError('%s must not be empty: %r' % (what, got))
    if shape is not None and got != shape:
        raise ValueError('%s is %r where %r is expected' % (what, got, shape))
    return got


class _MatrixStage(object):
    """A stage on a matrix that lies, or is put, on the device.  A subclass's __init__ makes its checks (host only), calls _open()
    (the device) and _resident() for every matrix; it defines result_device().  _noun is what the stage is called where an input
    lies on another device."""
    _noun = None

    def _open(self, device, like=None):
        """The device: `device` if given, else where `like` lies if it is a device tensor, else the current one.  -> torch."""
        from ._reader import _open_device
        if device is None and _is_device_tensor(like):
            device = like.device
        self._torch, _, self.L, self.device = _open_device(device, type(self).__name__)
        return self._torch

    def _resident(self, x, what):
        """A device tensor as it is (it must lie on this stage's device), a numpy array as a contiguous copy there."""
        if _is_device_tensor(x):
            if x.device != self.device:
                raise ValueError('%s are on %s, the %s runs on %s' % (what, x.device, self._noun, self.device))
            return x
        return self._torch.from_numpy(np.ascontiguousarray(x)).to(self.device)

    @staticmethod
    def _row_stride(t, T):
        """ld of a matrix of contiguous rows of T: a single row may carry any stride."""
        return int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), T)

    def _stream(self):
        return self._torch.cuda.current_stream(self.device).cuda_stream

    def _empty(self, shape, dtype):
        """An uninitialised tensor of torch's `dtype` (by name) on the device, allocated with that device current."""
        with self._torch.cuda.device(self.device):
            return self._torch.empty(shape, dtype=getattr(self._torch, dtype), device=self.device)

    def result(self, kind=None):
        """result_device(kind), or of the stage's default kind, as a numpy array."""
        return (self.result_device() if kind is None else self.result_device(kind)).cpu().numpy()
