"""ctypes binding of the sparse-GP conditional library (C ABI: include/zs_gp.h).

A library of its own, ``zhusuan-pytorch_amd/lib/libzs_gp.so`` (``make -C zhusuan-pytorch_amd/csrc gp``, run by
``__graft_entry__.build()``), loaded on the first kernel call of ``GPConditional``: ``import zhusuan`` imports neither this module
nor the library.  There is no fallback here: a missing library, or a tensor that is not resident on a HIP device, raises.

``zhusuan.distributions._gp_functions`` goes through the functions below, looked up on this module at call time.  They take
contiguous tensors -- ``x [N, d]``, ``inducing [M, d]``, ``lengthscale [d]``, ``amplitude [1]``, ``kzz_tril [M, M]``,
``fz [K, M]`` --, allocate the outputs and the workspaces the ABI asks for, and return them.  ``MAX_INDUCING`` (per element size)
and ``MAX_INPUT_DIM`` are the caps of the kernels (``zs_gp_max_inducing()`` / ``zs_gp_max_input_dim()``)."""
import ctypes
import os

import torch

from . import _binding, _hip

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libzs_gp.so")
ABI_VERSION = 1
MAX_INDUCING = {4: 128, 8: 64}
MAX_INPUT_DIM = 64
WS_PREP, WS_BWD = 0, 1

_p = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64

_PROTOTYPES = _binding.both({
    # kzz_tril, fz, Pf, prep, M, K, stream
    "zs_gp_prepare": [_p, _p, _i64, _p, _i64, _i64, _p],
    # x, inducing, lengthscale, amplitude, prep, mean, var, N, M, d, K, stream
    "zs_gp_moments": [_p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _p],
    # x, inducing, lengthscale, amplitude, Pf, prep, gmean, gvar, part, gx, ginducing, glengthscale, gamplitude, gtril, gfz,
    # N, M, d, K, shares, stream
    "zs_gp_moments_bwd": [_p, _p, _p, _p, _i64, _p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _p],
})
_PROTOTYPES["zs_gp_max_inducing"] = (_i, [_i])
_PROTOTYPES["zs_gp_max_input_dim"] = (_i, [])
_PROTOTYPES["zs_gp_row_shares"] = (_i64, [_i64])
_PROTOTYPES["zs_gp_workspace_elems"] = (_i64, [_i, _i64, _i64, _i64, _i64])        # which, M, d, K, n

_LIB = None


def GPLibrary(path):
    """A freshly loaded, uncached ``_binding.Library`` of the zs_gp_* C ABI from the file at ``path``; ``lib()`` keeps the
    in-tree one."""
    from .distributions import _gp_functions
    library = _binding.Library(path, who="zhusuan.distributions (sparse-GP conditional)", make_target="gp",
                               abi_symbol="zs_gp_abi_version", abi_version=ABI_VERSION, prototypes=_PROTOTYPES)
    caps = ({4: library.raw("zs_gp_max_inducing", 4), 8: library.raw("zs_gp_max_inducing", 8)}, library.raw("zs_gp_max_input_dim"))
    if not caps == (MAX_INDUCING, MAX_INPUT_DIM) == (_gp_functions.MAX_INDUCING, _gp_functions.MAX_INPUT_DIM):
        raise RuntimeError("%s takes (M, d) up to %s, zhusuan._gp_hip states %s and the distribution routes by %s: the three must "
                           "agree" % (path, caps, (MAX_INDUCING, MAX_INPUT_DIM), (_gp_functions.MAX_INDUCING, _gp_functions.MAX_INPUT_DIM)))
    return library


def lib(path=None):
    """The sparse-GP conditional library (lazy); ``path`` loads another file instead of the in-tree one and does not replace it."""
    return _binding.lazy_lib(globals(), GPLibrary, path)


def _sfx(dtype):
    return _binding.suffix(dtype, "zhusuan.distributions (sparse-GP conditional): the operands must be float32 or float64, got %s")


def _workspace(which, ref, M, d, K, n=1):
    elems = lib().raw("zs_gp_workspace_elems", which, M, d, K, n)
    if elems < 0:
        raise RuntimeError("zs_gp_workspace_elems rejected (which=%d, M=%d, d=%d, K=%d, n=%d)" % (which, M, d, K, n))
    return torch.empty(elems, dtype=ref.dtype, device=ref.device)


def _call(name, ref, operands, *args):
    _hip.require_device(ref, *operands)
    lib().call(name + _sfx(ref.dtype), *args, _hip.stream_for(ref))


def prepare(kzz_tril, fz):
    """``prep``: (L^-1)^T, c = L^-T L^-1 fz^T and L^-1 fz^T, padded to whole tiles (one launch of one workgroup)."""
    K, M = fz.shape
    prep = _workspace(WS_PREP, fz, M, 1, K)
    _call("zs_gp_prepare", fz, [kzz_tril], _hip.ptr(kzz_tril), _hip.ptr(fz), fz.numel(), _hip.ptr(prep), M, K)
    return prep


def moments(x, inducing, lengthscale, amplitude, prep, K):
    """(mean [K, N], var [N]) (one launch); nothing of size [N, M] is allocated."""
    (N, d), M = x.shape, inducing.shape[0]
    mean = torch.empty((K, N), dtype=x.dtype, device=x.device)
    var = torch.empty((N,), dtype=x.dtype, device=x.device)
    _call("zs_gp_moments", x, [inducing, lengthscale, amplitude, prep], _hip.ptr(x), _hip.ptr(inducing), _hip.ptr(lengthscale),
          _hip.ptr(amplitude), _hip.ptr(prep), _hip.ptr(mean), _hip.ptr(var), N, M, d, K)
    return mean, var


def moments_bwd(x, inducing, lengthscale, amplitude, prep, gmean, gvar, K, want_gx=True):
    """(gx [N, d] or None, ginducing [M, d], glengthscale [d], gamplitude [1], gtril [M, M], gfz [K, M]) from gmean [K, N] and
    gvar [N], either of which may be None (two launches)."""
    (N, d), M = x.shape, inducing.shape[0]
    shares = max(int(lib().raw("zs_gp_row_shares", N)), 1)
    part = _workspace(WS_BWD, x, M, d, K, shares)
    gx = torch.empty_like(x) if want_gx else None
    gZ, glen, gamp = torch.empty_like(inducing), torch.empty_like(lengthscale), torch.empty_like(amplitude)
    gL = torch.empty((M, M), dtype=x.dtype, device=x.device)
    gfz = torch.empty((K, M), dtype=x.dtype, device=x.device)
    _call("zs_gp_moments_bwd", x, [inducing, lengthscale, amplitude, prep, gmean, gvar], _hip.ptr(x), _hip.ptr(inducing),
          _hip.ptr(lengthscale), _hip.ptr(amplitude), K * M, _hip.ptr(prep), _hip.ptr(gmean), _hip.ptr(gvar), _hip.ptr(part),
          _hip.ptr(gx), _hip.ptr(gZ), _hip.ptr(glen), _hip.ptr(gamp), _hip.ptr(gL), _hip.ptr(gfz), N, M, d, K, shares)
    return gx, gZ, glen, gamp, gL, gfz
