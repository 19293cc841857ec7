"""ctypes binding of the multivariate-normal library (C ABI: include/zs_mvn.h).

A library of its own, ``zhusuan-pytorch_amd/lib/libzs_mvn.so`` (``make -C zhusuan-pytorch_amd/csrc mvn``, run by
``__graft_entry__.build()``), loaded on the first kernel call of ``MultivariateNormalCholesky``: ``import zhusuan`` and every
other family do not need it.  There is no fallback: a missing library, or a tensor that is not resident on a HIP device, raises.

``zhusuan.distributions._mvn_functions`` goes through the functions below, looked up on this module at call time.  They take
contiguous tensors -- ``mean`` as ``[R, D]``, ``tril`` as ``[R, D, D]``, per-particle operands as ``[K, R(, D)]`` -- allocate the
outputs and return them.  ``MAX_DIM`` is the widest row the kernels take (``zs_mvn_max_dim()``)."""
import ctypes
import os

import torch

from . import _binding, _hip

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libzs_mvn.so")
ABI_VERSION = 1
MAX_DIM = 64

_p = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64
_u64 = ctypes.c_uint64

_PROTOTYPES = _binding.both({
    # mean, tril, eps, z, lp, K, R, D, seed, call, rng_state, stream
    "zs_mvn_sample_logprob": [_p, _p, _p, _p, _p, _i64, _i64, _i64, _u64, _u64, _p, _p],
    # tril, eps, gz, glp, reparameterized, gmean, gtril, K, R, D, seed, call, rng_state, stream
    "zs_mvn_sample_logprob_bwd": [_p, _p, _p, _p, _i, _p, _p, _i64, _i64, _i64, _u64, _u64, _p, _p],
    # mean, tril, x, Px, lp, K, R, D, stream
    "zs_mvn_logprob": [_p, _p, _p, _i64, _p, _i64, _i64, _i64, _p],
    # mean, tril, x, Px, glp, gx, gmean, gtril, K, R, D, stream
    "zs_mvn_logprob_bwd": [_p, _p, _p, _i64, _p, _p, _p, _p, _i64, _i64, _i64, _p],
})
_PROTOTYPES["zs_mvn_max_dim"] = (_i, [])
_PROTOTYPES["zs_mvn_group_lanes"] = (_i, [_i64])          # D -> lanes per row

_LIB = None


def MvnLibrary(path):
    """A freshly loaded, uncached ``_binding.Library`` of the zs_mvn_* C ABI from the file at ``path``; ``lib()`` keeps the
    in-tree one."""
    return _binding.Library(path, who="zhusuan.distributions (multivariate normal)", make_target="mvn",
                            abi_symbol="zs_mvn_abi_version", abi_version=ABI_VERSION, prototypes=_PROTOTYPES)


def lib(path=None):
    """The multivariate-normal library (lazy); ``path`` loads another file instead of the in-tree one and does not replace it."""
    return _binding.lazy_lib(globals(), MvnLibrary, path)


def _sfx(dtype):
    return _binding.suffix(dtype, "zhusuan.distributions (multivariate normal): mean must be float32 or float64, got %s")


def _krd(tril, K):
    R, D, _ = tril.shape
    return int(K), int(R), int(D)


def _call(name, ref, operands, *args):
    _hip.require_device(ref, *operands)
    lib().call(name + _sfx(ref.dtype), *args, _hip.stream_for(ref))


def sample_logprob(mean, tril, K, eps=None, seed=0, call=0, rng_state=None):
    """V1: (z [K, R, D], lp [K, R]) in one launch."""
    K, R, D = _krd(tril, K)
    z = torch.empty((K, R, D), dtype=mean.dtype, device=mean.device)
    lp = torch.empty((K, R), dtype=mean.dtype, device=mean.device)
    _call("zs_mvn_sample_logprob", mean, [tril, eps, rng_state], _hip.ptr(mean), _hip.ptr(tril), _hip.ptr(eps), _hip.ptr(z),
          _hip.ptr(lp), K, R, D, _binding.u64(seed), _binding.u64(call), _hip.ptr(rng_state))
    return z, lp


def sample_logprob_bwd(tril, K, reparameterized, eps=None, seed=0, call=0, rng_state=None, gz=None, glp=None, want_gmean=True,
                       want_gtril=True):
    """Backward of V1: (gmean [R, D] or None, gtril [R, D, D] or None); ``eps`` None regenerates the draw's noise."""
    K, R, D = _krd(tril, K)
    gmean = torch.empty((R, D), dtype=tril.dtype, device=tril.device) if want_gmean else None
    gtril = torch.empty_like(tril) if want_gtril else None
    _call("zs_mvn_sample_logprob_bwd", tril, [eps, gz, glp, rng_state], _hip.ptr(tril), _hip.ptr(eps), _hip.ptr(gz), _hip.ptr(glp),
          int(bool(reparameterized)), _hip.ptr(gmean), _hip.ptr(gtril), K, R, D, _binding.u64(seed), _binding.u64(call),
          _hip.ptr(rng_state))
    return gmean, gtril


def logprob(mean, tril, K, x):
    """V2: lp [K, R] of x ([K, R, D] or [R, D])."""
    K, R, D = _krd(tril, K)
    lp = torch.empty((K, R), dtype=mean.dtype, device=mean.device)
    _call("zs_mvn_logprob", mean, [tril, x], _hip.ptr(mean), _hip.ptr(tril), _hip.ptr(x), x.numel(), _hip.ptr(lp), K, R, D)
    return lp


def logprob_bwd(mean, tril, K, x, glp, want_gx=True, want_gmean=True, want_gtril=True):
    """Backward of V2: (gx [K, R, D] or None, gmean [R, D] or None, gtril [R, D, D] or None)."""
    K, R, D = _krd(tril, K)
    gx = torch.empty((K, R, D), dtype=mean.dtype, device=mean.device) if want_gx else None
    gmean = torch.empty_like(mean) if want_gmean else None
    gtril = torch.empty_like(tril) if want_gtril else None
    _call("zs_mvn_logprob_bwd", mean, [tril, x, glp], _hip.ptr(mean), _hip.ptr(tril), _hip.ptr(x), x.numel(), _hip.ptr(glp),
          _hip.ptr(gx), _hip.ptr(gmean), _hip.ptr(gtril), K, R, D)
    return gx, gmean, gtril
