"""ctypes binding of the chain-diagnostics library (C ABI: include/zs_diag.h).

A library of its own, ``zhusuan-pytorch_amd/lib/libzs_diag.so`` (``make -C zhusuan-pytorch_amd/csrc diag``, run by
``__graft_entry__.build()``), loaded on the first call of ``zhusuan.diagnostics``: ``import zhusuan`` and the samplers do not need
it.  There is no fallback: a missing library, or a tensor that is not resident on a HIP device, raises.

``zhusuan.diagnostics`` goes through ``summary`` and ``autocorr`` below, looked up on this module at call time.  The operand is
handed over by address and two strides (``x[t st + c sc + e]``, in elements), never copied here: the caller has made sure that the
element axis is contiguous."""
import ctypes
import os

import torch

from . import _binding, _hip

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libzs_diag.so")
ABI_VERSION = 1
OUTPUTS = ("mean", "var_plus", "rhat", "ess", "lags", "capped")          # the order of the entry point's output pointers

_p = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64

_PROTOTYPES = _binding.both({
    # x, st, sc, T, C, E, split, max_lag, mean, var_plus, rhat, ess, lags, capped, stream
    "zs_diag_summary": [_p, _i64, _i64, _i64, _i64, _i64, _i, _i64, _p, _p, _p, _p, _p, _p, _p],
    # x, st, sc, T, C, E, L, acf, stream
    "zs_diag_autocorr": [_p, _i64, _i64, _i64, _i64, _i64, _i64, _p, _p],
})

_LIB = None


def DiagLibrary(path):
    """A freshly loaded, uncached ``_binding.Library`` of the zs_diag_* C ABI from the file at ``path``; ``lib()`` keeps the
    in-tree one."""
    return _binding.Library(path, who="zhusuan.diagnostics", make_target="diag", abi_symbol="zs_diag_abi_version",
                            abi_version=ABI_VERSION, prototypes=_PROTOTYPES)


def lib(path=None):
    """The chain-diagnostics library (lazy); ``path`` loads another file instead of the in-tree one and does not replace it."""
    return _binding.lazy_lib(globals(), DiagLibrary, path)


def _sfx(dtype):
    return _binding.suffix(dtype, "zhusuan.diagnostics: draws must be float32 or float64, got %s")


def summary(x, st, sc, T, C, E, split, max_lag, want=OUTPUTS):
    """One launch: ``(mean, var_plus, rhat, ess, lags, capped)``, each ``[E]`` (the last two int32) or None where its name is not
    in ``want``.  ``x``: a tensor whose first element is draw 0 of chain 0 of element 0; ``max_lag`` < 0: no cap."""
    _hip.require_device(x)
    sfx = _sfx(x.dtype)
    outs = [None if name not in want else torch.empty(E, dtype=torch.int32 if name in ("lags", "capped") else x.dtype, device=x.device)
            for name in OUTPUTS]
    lib().call("zs_diag_summary" + sfx, x.data_ptr(), int(st), int(sc), int(T), int(C), int(E), 1 if split else 0, int(max_lag),
               *([_hip.ptr(o) for o in outs] + [_hip.stream_for(x)]))
    return tuple(outs)


def autocorr(x, st, sc, T, C, E, L):
    """One launch: the autocorrelation of every unsplit chain at lags 0 .. L, ``[L + 1, C, E]``."""
    _hip.require_device(x)
    sfx = _sfx(x.dtype)
    acf = torch.empty((L + 1, C, E), dtype=x.dtype, device=x.device)
    lib().call("zs_diag_autocorr" + sfx, x.data_ptr(), int(st), int(sc), int(T), int(C), int(E), int(L), acf.data_ptr(), _hip.stream_for(x))
    return acf
