"""ctypes binding of the matrix-variate-normal library (C ABI: include/zs_matvar.h).

A library of its own, ``zhusuan-pytorch_amd/lib/libzs_matvar.so`` (``make -C zhusuan-pytorch_amd/csrc matvar``, run by
``__graft_entry__.build()``), loaded on the first kernel call of ``MatrixVariateNormalCholesky``: ``import zhusuan`` imports
neither this module nor the library.  There is no fallback here: a missing library, or a tensor that is not resident on a HIP
device, raises.

``zhusuan.distributions._matvar_functions`` goes through the functions below, looked up on this module at call time.  They take
contiguous tensors -- ``mean [R, n, p]``, ``u_tril [R, n, n]``, ``v_tril [R, p, p]``, per-particle operands ``[K, R(, n, p)]`` --,
allocate the outputs and the ``part`` workspace the ABI asks for, and return them.  ``MAX_DIM[element size]`` is the largest
``n`` and the largest ``p`` the kernels take (``zs_matvar_max_dim``)."""
import ctypes
import os

import torch

from . import _binding, _hip

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libzs_matvar.so")
ABI_VERSION = 1
MAX_DIM = {4: 128, 8: 64}
WS_SAMPLE_BWD, WS_LOGPROB_BWD = 0, 1

_p = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64
_u64 = ctypes.c_uint64

_PROTOTYPES = _binding.both({
    # mean, u_tril, v_tril, eps, z, lp, K, R, n, p, seed, call, rng_state, stream
    "zs_matvar_sample_logprob": [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _u64, _u64, _p, _p],
    # u_tril, v_tril, eps, gz, glp, part, gmean, gu, gv, K, R, n, p, seed, call, rng_state, stream
    "zs_matvar_sample_logprob_bwd": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _u64, _u64, _p, _p],
    # mean, u_tril, v_tril, x, Px, lp, K, R, n, p, stream
    "zs_matvar_logprob": [_p, _p, _p, _p, _i64, _p, _i64, _i64, _i64, _i64, _p],
    # mean, u_tril, v_tril, x, Px, glp, part, gx, gmean, gu, gv, K, R, n, p, stream
    "zs_matvar_logprob_bwd": [_p, _p, _p, _p, _i64, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _p],
})
_PROTOTYPES["zs_matvar_max_dim"] = (_i, [_i])                                            # elem_bytes
_PROTOTYPES["zs_matvar_shares"] = (_i64, [_i64, _i64])                                   # K, R
_PROTOTYPES["zs_matvar_workspace_elems"] = (_i64, [_i, _i, _i64, _i64, _i64, _i64])      # which, elem_bytes, K, R, n, p

_LIB = None


def MatvarLibrary(path):
    """A freshly loaded, uncached ``_binding.Library`` of the zs_matvar_* C ABI from the file at ``path``; ``lib()`` keeps the
    in-tree one."""
    from .distributions import _matvar_functions
    library = _binding.Library(path, who="zhusuan.distributions (matrix-variate normal)", make_target="matvar",
                               abi_symbol="zs_matvar_abi_version", abi_version=ABI_VERSION, prototypes=_PROTOTYPES)
    caps = {nb: library.raw("zs_matvar_max_dim", nb) for nb in (4, 8)}
    if not caps == MAX_DIM == _matvar_functions.MAX_DIM:
        raise RuntimeError("%s takes events up to %s, zhusuan._matvar_hip.MAX_DIM is %s and the distribution routes by %s: the "
                           "three must agree" % (path, caps, MAX_DIM, _matvar_functions.MAX_DIM))
    for K, R in ((1, 1), (5, 1), (50, 1), (5, 64), (17, 3), (300, 40), (2, 1000)):
        if library.raw("zs_matvar_shares", K, R) != _matvar_functions.shares(K, R):
            raise RuntimeError("%s cuts K = %d particles of R = %d rows into %d shares, the distribution's routing assumes %d"
                               % (path, K, R, library.raw("zs_matvar_shares", K, R), _matvar_functions.shares(K, R)))
    return library


def lib(path=None):
    """The matrix-variate-normal library (lazy); ``path`` loads another file instead of the in-tree one and does not replace it."""
    return _binding.lazy_lib(globals(), MatvarLibrary, path)


def _sfx(dtype):
    return _binding.suffix(dtype, "zhusuan.distributions (matrix-variate normal): mean must be float32 or float64, got %s")


def _dims(mean, K):
    R, n, p = mean.shape
    return int(K), int(R), int(n), int(p)


def workspace(which, ref, K, R, n, p):
    """An uninitialised ``part`` workspace of the size ``zs_matvar_workspace_elems`` states, like ``ref``."""
    count = lib().raw("zs_matvar_workspace_elems", which, ref.element_size(), K, R, n, p)
    if count < 0:
        raise RuntimeError("zs_matvar_workspace_elems rejected (which=%d, K=%d, R=%d, n=%d, p=%d)" % (which, K, R, n, p))
    return torch.empty(count, dtype=ref.dtype, device=ref.device)


def _call(name, ref, operands, *args):
    _hip.require_device(ref, *operands)
    lib().call(name + _sfx(ref.dtype), *args, _hip.stream_for(ref))


def _like(ref, want):
    return torch.empty_like(ref) if want else None


def sample_logprob(mean, u, v, K, eps=None, seed=0, call=0, rng_state=None):
    """M1: (z [K, R, n, p], lp [K, R]) in one launch."""
    K, R, n, p = _dims(mean, K)
    z = torch.empty((K, R, n, p), dtype=mean.dtype, device=mean.device)
    lp = torch.empty((K, R), dtype=mean.dtype, device=mean.device)
    _call("zs_matvar_sample_logprob", mean, [u, v, eps, rng_state], _hip.ptr(mean), _hip.ptr(u), _hip.ptr(v), _hip.ptr(eps),
          _hip.ptr(z), _hip.ptr(lp), K, R, n, p, _binding.u64(seed), _binding.u64(call), _hip.ptr(rng_state))
    return z, lp


def sample_logprob_bwd(mean, u, v, K, eps=None, seed=0, call=0, rng_state=None, gz=None, glp=None, want=(True, True, True)):
    """Backward of M1: (gmean, gu, gv), None where ``want`` is False; ``eps`` None regenerates the draw's noise.  ``mean`` gives
    the shape only."""
    K, R, n, p = _dims(mean, K)
    part = workspace(WS_SAMPLE_BWD, u, K, R, n, p) if gz is not None else None
    gmean, gu, gv = _like(mean, want[0]), _like(u, want[1]), _like(v, want[2])
    _call("zs_matvar_sample_logprob_bwd", u, [v, eps, gz, glp, rng_state], _hip.ptr(u), _hip.ptr(v), _hip.ptr(eps), _hip.ptr(gz),
          _hip.ptr(glp), _hip.ptr(part), _hip.ptr(gmean), _hip.ptr(gu), _hip.ptr(gv), K, R, n, p, _binding.u64(seed),
          _binding.u64(call), _hip.ptr(rng_state))
    return gmean, gu, gv


def logprob(mean, u, v, K, x):
    """M2: lp [K, R] of x ([K, R, n, p] or [R, n, p]) in one launch."""
    K, R, n, p = _dims(mean, K)
    lp = torch.empty((K, R), dtype=mean.dtype, device=mean.device)
    _call("zs_matvar_logprob", mean, [u, v, x], _hip.ptr(mean), _hip.ptr(u), _hip.ptr(v), _hip.ptr(x), x.numel(), _hip.ptr(lp),
          K, R, n, p)
    return lp


def logprob_bwd(mean, u, v, K, x, glp, want_gx=True, want=(True, True, True)):
    """Backward of M2: (gx [K, R, n, p], gmean, gu, gv), None where not wanted."""
    K, R, n, p = _dims(mean, K)
    part = workspace(WS_LOGPROB_BWD, mean, K, R, n, p) if any(want) else None
    gx = torch.empty((K, R, n, p), dtype=mean.dtype, device=mean.device) if want_gx else None
    gmean, gu, gv = _like(mean, want[0]), _like(u, want[1]), _like(v, want[2])
    _call("zs_matvar_logprob_bwd", mean, [u, v, x, glp], _hip.ptr(mean), _hip.ptr(u), _hip.ptr(v), _hip.ptr(x), x.numel(),
          _hip.ptr(glp), _hip.ptr(part), _hip.ptr(gx), _hip.ptr(gmean), _hip.ptr(gu), _hip.ptr(gv), K, R, n, p)
    return gx, gmean, gu, gv
