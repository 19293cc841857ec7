"""ctypes binding of the low-rank multivariate-normal library (C ABI: include/zs_lowrank.h).

A library of its own, ``zhusuan-pytorch_amd/lib/libzs_lowrank.so`` (``make -C zhusuan-pytorch_amd/csrc lowrank``, run by
``__graft_entry__.build()``), loaded on the first kernel call of ``MultivariateNormalLowRank``: ``import zhusuan`` imports neither
this module nor the library.  There is no fallback here: a missing library, or a tensor that is not resident on a HIP device,
raises.

``zhusuan.distributions._lowrank_functions`` goes through the functions below, looked up on this module at call time.  They take
contiguous tensors -- ``mean [R, D]``, ``factor [R, D, r]``, ``diag [R, D]``, per-particle operands ``[K, R(, D)]`` --, allocate
the outputs and the workspaces the ABI asks for, and return them.  ``MAX_DIM`` / ``MAX_RANK`` are the caps of the kernels
(``zs_lowrank_max_dim()`` / ``zs_lowrank_max_rank()``)."""
import ctypes
import os

import torch

from . import _binding, _hip

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libzs_lowrank.so")
ABI_VERSION = 1
MAX_DIM = 65536
MAX_RANK = 64
WS_PREP, WS_PREPARE, WS_LOGPROB_BWD = 0, 1, 2

_p = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64
_u64 = ctypes.c_uint64

_PROTOTYPES = _binding.both({
    # factor, diag, part, prep, R, D, r, splits, stream
    "zs_lowrank_prepare": [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _p],
    # mean, factor, diag, prep, x, Px, lp, K, R, D, r, stream
    "zs_lowrank_logprob": [_p, _p, _p, _p, _p, _i64, _p, _i64, _i64, _i64, _i64, _p],
    # mean, factor, diag, prep, x, Px, glp, part, gx, gmean, gfactor, gdiag, K, R, D, r, shares, stream
    "zs_lowrank_logprob_bwd": [_p, _p, _p, _p, _p, _i64, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _p],
    # mean, factor, diag, eps, z, K, R, D, r, seed, call, rng_state, stream
    "zs_lowrank_sample": [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _u64, _u64, _p, _p],
    # diag, eps, gz, gmean, gfactor, gdiag, K, R, D, r, seed, call, rng_state, stream
    "zs_lowrank_sample_bwd": [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _u64, _u64, _p, _p],
})
_PROTOTYPES["zs_lowrank_max_dim"] = (_i, [])
_PROTOTYPES["zs_lowrank_max_rank"] = (_i, [])
_PROTOTYPES["zs_lowrank_splits"] = (_i64, [_i, _i64, _i64, _i64])                       # which, K, R, D
_PROTOTYPES["zs_lowrank_workspace_elems"] = (_i64, [_i, _i64, _i64, _i64, _i64])        # which, R, D, r, n

_LIB = None


def LowRankLibrary(path):
    """A freshly loaded, uncached ``_binding.Library`` of the zs_lowrank_* C ABI from the file at ``path``; ``lib()`` keeps the
    in-tree one."""
    from .distributions import _lowrank_functions
    library = _binding.Library(path, who="zhusuan.distributions (low-rank multivariate normal)", make_target="lowrank",
                               abi_symbol="zs_lowrank_abi_version", abi_version=ABI_VERSION, prototypes=_PROTOTYPES)
    caps = (library.raw("zs_lowrank_max_dim"), library.raw("zs_lowrank_max_rank"))
    if not caps == (MAX_DIM, MAX_RANK) == (_lowrank_functions.MAX_DIM, _lowrank_functions.MAX_RANK):
        raise RuntimeError("%s takes (D, r) up to %s, zhusuan._lowrank_hip states %s and the distribution routes by %s: the three "
                           "must agree" % (path, caps, (MAX_DIM, MAX_RANK), (_lowrank_functions.MAX_DIM, _lowrank_functions.MAX_RANK)))
    return library


def lib(path=None):
    """The low-rank multivariate-normal library (lazy); ``path`` loads another file instead of the in-tree one and does not
    replace it."""
    return _binding.lazy_lib(globals(), LowRankLibrary, path)


def _sfx(dtype):
    return _binding.suffix(dtype, "zhusuan.distributions (low-rank multivariate normal): the parameters must be float32 or "
                                  "float64, got %s")


def _workspace(which, ref, R, D, r, n=1):
    elems = lib().raw("zs_lowrank_workspace_elems", which, R, D, r, n)
    if elems < 0:
        raise RuntimeError("zs_lowrank_workspace_elems rejected (which=%d, R=%d, D=%d, r=%d, n=%d)" % (which, R, D, r, n))
    return torch.empty(elems, dtype=ref.dtype, device=ref.device)


def _call(name, ref, operands, *args):
    _hip.require_device(ref, *operands)
    lib().call(name + _sfx(ref.dtype), *args, _hip.stream_for(ref))


def prepare(factor, diag):
    """``prep``: per row the inverse Cholesky factor of the capacitance, its inverse and the two log-determinants (two
    launches); it serves every density call of the same (factor, diag)."""
    R, D, r = factor.shape
    splits = max(int(lib().raw("zs_lowrank_splits", WS_PREPARE, 0, R, D)), 1)
    part, prep = _workspace(WS_PREPARE, factor, R, D, r, splits), _workspace(WS_PREP, factor, R, D, r)
    _call("zs_lowrank_prepare", factor, [diag], _hip.ptr(factor), _hip.ptr(diag), _hip.ptr(part), _hip.ptr(prep), R, D, r, splits)
    return prep


def logprob(mean, factor, diag, prep, x, K):
    """lp [K, R] of x ([K, R, D] or [R, D])."""
    R, D, r = factor.shape
    lp = torch.empty((K, R), dtype=mean.dtype, device=mean.device)
    _call("zs_lowrank_logprob", mean, [factor, diag, prep, x], _hip.ptr(mean), _hip.ptr(factor), _hip.ptr(diag), _hip.ptr(prep),
          _hip.ptr(x), x.numel(), _hip.ptr(lp), K, R, D, r)
    return lp


def logprob_bwd(mean, factor, diag, prep, x, glp, K, want_gx=True):
    """(gx [K, R, D] or None, gmean [R, D], gfactor [R, D, r], gdiag [R, D]) (two launches)."""
    R, D, r = factor.shape
    shares = max(int(lib().raw("zs_lowrank_splits", WS_LOGPROB_BWD, K, R, D)), 1)
    part = _workspace(WS_LOGPROB_BWD, mean, R, D, r, shares)
    gx = torch.empty((K, R, D), dtype=mean.dtype, device=mean.device) if want_gx else None
    gmean, gfactor, gdiag = torch.empty_like(mean), torch.empty_like(factor), torch.empty_like(diag)
    _call("zs_lowrank_logprob_bwd", mean, [factor, diag, prep, x, glp], _hip.ptr(mean), _hip.ptr(factor), _hip.ptr(diag),
          _hip.ptr(prep), _hip.ptr(x), x.numel(), _hip.ptr(glp), _hip.ptr(part), _hip.ptr(gx), _hip.ptr(gmean), _hip.ptr(gfactor),
          _hip.ptr(gdiag), K, R, D, r, shares)
    return gx, gmean, gfactor, gdiag


def sample(mean, factor, diag, K, eps=None, seed=0, call=0, rng_state=None):
    """z [K, R, D]; ``eps`` [K, R, D + r] replaces the Philox stream of (seed, call, rng_state)."""
    R, D, r = factor.shape
    z = torch.empty((K, R, D), dtype=mean.dtype, device=mean.device)
    _call("zs_lowrank_sample", mean, [factor, diag, eps, rng_state], _hip.ptr(mean), _hip.ptr(factor), _hip.ptr(diag), _hip.ptr(eps),
          _hip.ptr(z), K, R, D, r, _binding.u64(seed), _binding.u64(call), _hip.ptr(rng_state))
    return z


def sample_bwd(factor, diag, gz, K, eps=None, seed=0, call=0, rng_state=None):
    """(gmean [R, D], gfactor [R, D, r], gdiag [R, D]) of the draw; ``eps`` None regenerates its noise."""
    R, D, r = factor.shape
    gmean, gfactor, gdiag = torch.empty_like(diag), torch.empty_like(factor), torch.empty_like(diag)
    _call("zs_lowrank_sample_bwd", diag, [eps, gz, rng_state], _hip.ptr(diag), _hip.ptr(eps), _hip.ptr(gz), _hip.ptr(gmean),
          _hip.ptr(gfactor), _hip.ptr(gdiag), K, R, D, r, _binding.u64(seed), _binding.u64(call), _hip.ptr(rng_state))
    return gmean, gfactor, gdiag
