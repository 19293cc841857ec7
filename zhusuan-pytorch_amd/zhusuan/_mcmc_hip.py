"""ctypes binding of the stochastic-gradient MCMC update library (C ABI: include/zs_mcmc.h).

A library of its own, ``zhusuan-pytorch_amd/lib/libzs_mcmc.so`` (``make -C zhusuan-pytorch_amd/csrc mcmc``, run by
``__graft_entry__.build()``), loaded on the first update: ``import zhusuan`` and the variational path do not need it.
There is no fallback: a missing library, or a tensor that is not resident on a HIP device, raises.

Every update of ``zhusuan.mcmc`` goes through ``update()`` below, looked up on this module at call time.
"""
import ctypes
import os

import torch

from . import _hip

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libzs_mcmc.so")
ABI_VERSION = 1
MAX_TENSORS = 32          # ZS_MCMC_MAX_TENSORS

SGLD, PSGLD, SGHMC_PRE, SGHMC_POST = 0, 1, 2, 3
SECOND_ORDER, RESAMPLE_V = 1, 2

_p = ctypes.c_void_p
_d = ctypes.c_double


class McmcTensor(ctypes.Structure):          # struct zs_mcmc_tensor
    _fields_ = [("q_in", _p), ("q_out", _p), ("grad", _p), ("state", _p), ("z", _p), ("start", ctypes.c_int64)]


_ARGTYPES = [ctypes.c_int, _p, ctypes.c_int, ctypes.c_int64, _d, _d, _d, _d, _d, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64,
             _p, _p]
_ERRORS = {-1: "invalid argument (ZS_EINVAL)", -2: "not supported (ZS_ENOTSUP)"}


class McmcLibrary(object):
    """A loaded shared object exporting the zs_mcmc_* C ABI (binding the symbols needs no GPU)."""

    def __init__(self, path=None):
        path = path or LIB_PATH
        if not os.path.exists(path):
            raise RuntimeError(
                "zhusuan.mcmc (MI355X build): sampler kernel library not found at %s -- run "
                "`make -C zhusuan-pytorch_amd/csrc mcmc` (or `python -c 'import __graft_entry__ as g; g.build()'`). "
                "There is no CPU fallback." % path)
        self.path = path
        self.cdll = ctypes.CDLL(path)
        self.cdll.zs_mcmc_abi_version.restype = ctypes.c_int
        self.cdll.zs_mcmc_abi_version.argtypes = []
        got = self.cdll.zs_mcmc_abi_version()
        if got != ABI_VERSION:
            raise RuntimeError("zhusuan.mcmc: %s has ABI version %d, expected %d" % (path, got, ABI_VERSION))
        self._fn = {}
        for name in ("zs_mcmc_update_f32", "zs_mcmc_update_f64"):
            fn = getattr(self.cdll, name)
            fn.restype = ctypes.c_int
            fn.argtypes = _ARGTYPES
            self._fn[name] = fn

    def raw(self, name, *args):
        """The entry point's own return code (0 = ok)."""
        return self._fn[name](*args)

    def call(self, name, *args):
        rc = self._fn[name](*args)
        if rc != 0:
            raise RuntimeError("%s failed with code %d: %s" % (name, rc, _ERRORS.get(rc, "HIP error")))


_LIB = None


def lib(path=None):
    """The sampler library (lazy); ``path`` loads another file instead of the in-tree one and does not replace it."""
    global _LIB
    if path is not None:
        return McmcLibrary(path)
    if _LIB is None:
        _LIB = McmcLibrary(LIB_PATH)
    return _LIB


def _entry(dtype):
    if dtype == torch.float32:
        return "zs_mcmc_update_f32"
    if dtype == torch.float64:
        return "zs_mcmc_update_f64"
    raise RuntimeError("zhusuan.mcmc: latents must be float32 or float64, got %s" % dtype)


def update(kind, q_in, q_out, grad=None, state=None, z=None, lr=0., decay=0., epsilon=0., alpha=0., beta=0., flags=0,
           seed=0, call=0, rng_state=None, library=None):
    """One launch of the fused update over the tensors of ``q_in`` (a list of at most MAX_TENSORS contiguous tensors of one
    dtype on one HIP device).  ``q_out``: where the updated values go (may be the same tensors); ``grad`` / ``state``:
    lists like ``q_in`` or None where the kind does not read them; ``z``: None, or a list whose entries are injected
    standard normals or None (drawn in-kernel from Philox (seed, call), or from ``rng_state`` + call).  The flat index space
    of the launch is the tensors in list order."""
    k = len(q_in)
    table = (McmcTensor * max(k, 1))()
    every = []
    start = 0
    for i in range(k):
        row = (q_in[i], q_out[i], grad[i] if grad is not None else None, state[i] if state is not None else None,
               z[i] if z is not None else None)
        for t in row:
            if t is None:
                continue
            if t.dtype != q_in[0].dtype or t.numel() != q_in[i].numel() or not t.is_contiguous():
                raise RuntimeError("zhusuan.mcmc: operands of one latent must be contiguous, of one dtype and one size")
            every.append(t)
        e = table[i]
        e.q_in, e.q_out, e.grad, e.state, e.z = [_hip.ptr(t) for t in row]
        e.start = start
        start += q_in[i].numel()
    if k == 0:
        return
    _hip.require_device(*(every + [rng_state]))
    (library or lib()).call(_entry(q_in[0].dtype), int(kind), table, k, start, float(lr), float(decay), float(epsilon),
                            float(alpha), float(beta), int(flags), int(seed) & 0xFFFFFFFFFFFFFFFF, int(call) & 0xFFFFFFFFFFFFFFFF,
                            _hip.ptr(rng_state), _hip.stream_for(q_in[0]))
