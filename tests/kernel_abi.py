"""What every tests/test_<lib>_kernel.py needs to drive a satellite library's raw C ABI: the constants, pointer / stream /
suffix helpers, the loaders, bit comparison, and `Arena` -- operands inside guarded buffers, which is what holds every kernel
to its bounds and runs it on both its 16-byte and its element path.  tests/test_kernel_abi_helpers.py tests this file (CPU)."""
import importlib

import numpy as np
import torch

DEV = "cuda:0"
EINVAL, ENOTSUP = -1, -2
GUARD = 4          # fill elements kept on both sides of every operand: 16 bytes of float32, 32 of float64 / int64
SENTINEL = 777.0
F32, F64, I64 = torch.float32, torch.float64, torch.int64


def ptr(t):
    """None -> NULL, an int -> that raw address, a tensor -> its data pointer"""
    return None if t is None else (t if isinstance(t, int) else t.data_ptr())


def stream():
    from zhusuan import _hip
    return _hip.stream_for(torch.empty(0, device=DEV))


def sfx(dtype):
    return "_f32" if dtype == F32 else "_f64"


def unit(dtype):
    return 2.0 ** -24 if dtype == F32 else 2.0 ** -53


def load(binding):
    """A fresh handle on a satellite library: load("cat") is _cat_hip.lib(_cat_hip.LIB_PATH)."""
    mod = importlib.import_module("zhusuan._%s_hip" % binding)
    return mod.lib(mod.LIB_PATH)


def load_main():
    from zhusuan import _hip
    return _hip.KernelLibrary(_hip.LIB_PATH)


def same_bits(a, b):
    """The same shape and the same bit patterns (-0.0 is not +0.0, a NaN equals the NaN of the same payload); integer tensors by
    value; None only equals None."""
    if a is None or b is None:
        return a is None and b is None
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.dtype.is_floating_point:
        return torch.equal(a, b)
    it = torch.int32 if a.dtype == F32 else torch.int64
    return torch.equal(a.view(it), b.view(it))


def _is_fill(t, fill):
    """elementwise: t still holds `fill` (a NaN fill by isnan; an integer tensor holds int(fill))"""
    if fill != fill:
        return torch.isnan(t)
    return t == (fill if t.dtype.is_floating_point else int(fill))


def untouched(v, fill=SENTINEL):
    """Every element of v still holds the fill."""
    return bool(_is_fill(v, fill).all())


def covered(outs, fill=SENTINEL):
    """No element of an output keeps the fill its buffer was created with."""
    for t in outs:
        if t is None:
            continue
        assert not bool(_is_fill(t, fill).any()), "an output element was never written"


class Arena(object):
    """Operands, each inside its own buffer: GUARD fill elements, `shift` more (0: the data is 16-byte aligned, 1: it is not),
    the data, GUARD fill elements.  `dtype` is the default of put() and out(); an integer buffer is filled with int(fill)."""

    def __init__(self, shift=0, fill=SENTINEL, dtype=None, device=DEV):
        self.shift, self.fill, self.dtype, self.device = shift, fill, dtype, device
        self.bufs, self.outs = [], []          # (buffer, offset of the data, its length): every operand, the outputs

    def _view(self, shape, dtype, is_out):
        n = int(np.prod(shape))
        o = GUARD + self.shift
        fill = self.fill if dtype.is_floating_point else int(self.fill)          # (int() of a NaN raises)
        buf = torch.full((o + n + GUARD,), fill, dtype=dtype, device=self.device)
        self.bufs.append((buf, o, n))
        if is_out:
            self.outs.append((buf, o, n))
        return buf[o:o + n].view(shape)

    def put(self, a, dtype=None):
        """A copy of a tensor or numpy array in `dtype` (else the arena's, else its own), as a view of its shape; None -> None."""
        if a is None:
            return None
        t = torch.from_numpy(np.ascontiguousarray(a)) if isinstance(a, np.ndarray) else a
        dtype = dtype if dtype is not None else (self.dtype if self.dtype is not None else t.dtype)
        v = self._view(tuple(t.shape), dtype, False)
        v.copy_(t.to(dtype))
        return v

    def out(self, shape, dtype=None):
        """An output that holds the fill: a flat view of `shape` elements, or a view of the tuple `shape`."""
        shape = (shape,) if isinstance(shape, int) else tuple(shape)
        return self._view(shape, dtype if dtype is not None else self.dtype, True)

    def check_guards(self):
        """After the device has finished: the guards of every operand, inputs included, still hold the fill."""
        if torch.device(self.device).type == "cuda":
            torch.cuda.synchronize()
        for buf, o, n in self.bufs:
            assert untouched(torch.cat([buf[:o], buf[o + n:]]), self.fill), "write outside the tensor"

    def untouched(self):
        """No output buffer, guards included, was written."""
        return all(untouched(buf, self.fill) for buf, _, _ in self.outs)
