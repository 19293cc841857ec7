"""ctypes binding of the categorical library (C ABI: include/zs_cat.h).

A library of its own, ``zhusuan-pytorch_amd/lib/libzs_cat.so`` (``make -C zhusuan-pytorch_amd/csrc cat``, run by
``__graft_entry__.build()``), loaded on the first categorical kernel call: ``import zhusuan`` and every other family do not need
it.  There is no fallback: a missing library, or a tensor that is not resident on a HIP device, raises.

``zhusuan.distributions._cat_functions`` goes through the functions below, looked up on this module at call time.  They take
contiguous tensors -- ``logits`` as ``[R, N]``, per-particle operands as ``[K, R(, N)]`` -- allocate the outputs and return them.
"""
import ctypes
import os

import torch

from . import _binding, _hip

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libzs_cat.so")
ABI_VERSION = 1

_p = ctypes.c_void_p
_d = ctypes.c_double
_i = ctypes.c_int
_i64 = ctypes.c_int64
_u64 = ctypes.c_uint64

_PROTOTYPES = _binding.both({
    # x, out, n, stream
    "zs_cat_exp": [_p, _p, _i64, _p],
    # logits, u, idx, onehot, lp, K, R, N, seed, call, rng_state, stream
    "zs_cat_sample_logprob": [_p, _p, _p, _p, _p, _i64, _i64, _i64, _u64, _u64, _p, _p],
    # logits, idx, x, Px, lp, K, R, N, stream
    "zs_cat_logprob": [_p, _p, _p, _i64, _p, _i64, _i64, _i64, _p],
    # logits, idx, x, Px, glp, glogits, gx, K, R, N, stream
    "zs_cat_logprob_bwd": [_p, _p, _p, _i64, _p, _p, _p, _i64, _i64, _i64, _p],
    # logits, u, tau, exp_space, y, ey, lp, K, R, N, seed, call, rng_state, stream
    "zs_cat_expconcrete_sample_logprob": [_p, _p, _d, _i, _p, _p, _p, _i64, _i64, _i64, _u64, _u64, _p, _p],
    # logits, y, tau, exp_space, gy, gey, glp, glogits, K, R, N, stream
    "zs_cat_expconcrete_sample_logprob_bwd": [_p, _p, _d, _i, _p, _p, _p, _p, _i64, _i64, _i64, _p],
    # logits, y, Py, tau, exp_space, lp, K, R, N, stream
    "zs_cat_expconcrete_logprob": [_p, _p, _i64, _d, _i, _p, _i64, _i64, _i64, _p],
    # logits, y, Py, tau, exp_space, glp, gy, glogits, K, R, N, stream
    "zs_cat_expconcrete_logprob_bwd": [_p, _p, _i64, _d, _i, _p, _p, _p, _i64, _i64, _i64, _p],
})
_PROTOTYPES["zs_cat_group_lanes"] = (_i, [_i64])          # N -> lanes per row

_LIB = None


def CatLibrary(path):
    """A freshly loaded, uncached ``_binding.Library`` of the zs_cat_* C ABI from the file at ``path``; ``lib()`` keeps the
    in-tree one."""
    return _binding.Library(path, who="zhusuan.distributions (categorical)", make_target="cat", abi_symbol="zs_cat_abi_version",
                            abi_version=ABI_VERSION, prototypes=_PROTOTYPES)


def lib(path=None):
    """The categorical library (lazy); ``path`` loads another file instead of the in-tree one and does not replace it."""
    return _binding.lazy_lib(globals(), CatLibrary, path)


def _sfx(dtype):
    return _binding.suffix(dtype, "zhusuan.distributions (categorical): logits must be float32 or float64, got %s")


def _krn(logits, K):
    R, N = logits.shape
    return int(K), int(R), int(N)


def _call(name, logits, operands, *args):
    _hip.require_device(logits, *operands)
    lib().call(name + _sfx(logits.dtype), *args, _hip.stream_for(logits))


def sample_logprob(logits, K, u=None, seed=0, call=0, rng_state=None, want_index=True, want_onehot=False):
    """C1: (idx int64[K, R] or None, onehot [K, R, N] or None, lp [K, R]) in one launch."""
    K, R, N = _krn(logits, K)
    idx = torch.empty((K, R), dtype=torch.int64, device=logits.device) if want_index else None
    onehot = torch.empty((K, R, N), dtype=logits.dtype, device=logits.device) if want_onehot else None
    lp = torch.empty((K, R), dtype=logits.dtype, device=logits.device)
    _call("zs_cat_sample_logprob", logits, [u, rng_state], _hip.ptr(logits), _hip.ptr(u), _hip.ptr(idx), _hip.ptr(onehot),
          _hip.ptr(lp), K, R, N, _binding.u64(seed), _binding.u64(call), _hip.ptr(rng_state))
    return idx, onehot, lp


def logprob(logits, K, idx=None, x=None):
    """C2: lp [K, R] of indices (int64 [K, R] or [R]) or of weights ([K, R, N] or [R, N])."""
    K, R, N = _krn(logits, K)
    v = idx if x is None else x
    lp = torch.empty((K, R), dtype=logits.dtype, device=logits.device)
    _call("zs_cat_logprob", logits, [v], _hip.ptr(logits), _hip.ptr(idx), _hip.ptr(x), v.numel(), _hip.ptr(lp), K, R, N)
    return lp


def logprob_bwd(logits, K, glp, idx=None, x=None, want_gx=False):
    """Backward of C2: (glogits [R, N], gx [K, R, N] or None)."""
    K, R, N = _krn(logits, K)
    v = idx if x is None else x
    glogits = torch.empty_like(logits)
    gx = torch.empty((K, R, N), dtype=logits.dtype, device=logits.device) if want_gx else None
    _call("zs_cat_logprob_bwd", logits, [v, glp], _hip.ptr(logits), _hip.ptr(idx), _hip.ptr(x), v.numel(), _hip.ptr(glp),
          _hip.ptr(glogits), _hip.ptr(gx), K, R, N)
    return glogits, gx


def relaxed_sample_logprob(logits, K, tau, exp_space, u=None, seed=0, call=0, rng_state=None):
    """C3: (y [K, R, N], exp(y) or None, lp [K, R]) in one launch."""
    K, R, N = _krn(logits, K)
    y = torch.empty((K, R, N), dtype=logits.dtype, device=logits.device)
    ey = torch.empty_like(y) if exp_space else None
    lp = torch.empty((K, R), dtype=logits.dtype, device=logits.device)
    _call("zs_cat_expconcrete_sample_logprob", logits, [u, rng_state], _hip.ptr(logits), _hip.ptr(u), float(tau), int(bool(exp_space)),
          _hip.ptr(y), _hip.ptr(ey), _hip.ptr(lp), K, R, N, _binding.u64(seed), _binding.u64(call), _hip.ptr(rng_state))
    return y, ey, lp


def relaxed_sample_logprob_bwd(logits, K, tau, exp_space, y, gy=None, gey=None, glp=None):
    """Backward of C3 from the saved y: glogits [R, N]."""
    K, R, N = _krn(logits, K)
    glogits = torch.empty_like(logits)
    _call("zs_cat_expconcrete_sample_logprob_bwd", logits, [y, gy, gey, glp], _hip.ptr(logits), _hip.ptr(y), float(tau),
          int(bool(exp_space)), _hip.ptr(gy), _hip.ptr(gey), _hip.ptr(glp), _hip.ptr(glogits), K, R, N)
    return glogits


def relaxed_logprob(logits, K, tau, exp_space, y):
    """C4: lp [K, R] of y ([K, R, N] or [R, N])."""
    K, R, N = _krn(logits, K)
    lp = torch.empty((K, R), dtype=logits.dtype, device=logits.device)
    _call("zs_cat_expconcrete_logprob", logits, [y], _hip.ptr(logits), _hip.ptr(y), y.numel(), float(tau), int(bool(exp_space)),
          _hip.ptr(lp), K, R, N)
    return lp


def relaxed_logprob_bwd(logits, K, tau, exp_space, y, glp, want_gy=True, want_glogits=True):
    """Backward of C4: (gy [K, R, N] or None, glogits [R, N] or None)."""
    K, R, N = _krn(logits, K)
    gy = torch.empty((K, R, N), dtype=logits.dtype, device=logits.device) if want_gy else None
    glogits = torch.empty_like(logits) if want_glogits else None
    _call("zs_cat_expconcrete_logprob_bwd", logits, [y, glp], _hip.ptr(logits), _hip.ptr(y), y.numel(), float(tau),
          int(bool(exp_space)), _hip.ptr(glp), _hip.ptr(gy), _hip.ptr(glogits), K, R, N)
    return gy, glogits
