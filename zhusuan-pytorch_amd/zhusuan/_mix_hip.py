"""ctypes binding of the mixture-of-Gaussians library (C ABI: include/zs_mix.h).

A library of its own, ``zhusuan-pytorch_amd/lib/libzs_mix.so`` (``make -C zhusuan-pytorch_amd/csrc mix``, run by
``__graft_entry__.build()``), loaded on the first kernel call of ``NormalMixture``: ``import zhusuan`` imports neither this module
nor the library.  There is no fallback here: a missing library, or a tensor that is not resident on a HIP device, raises.

``zhusuan.distributions._mix_functions`` goes through the functions below, looked up on this module at call time.  They take
contiguous tensors -- ``logits [C]``, ``mean [C, D]``, ``logstd [C, D]``, ``x [R, D]``, ``g [R]`` --, allocate the outputs and the
workspaces the ABI asks for, and return them.  ``MAX_DIM`` / ``MAX_COMPONENTS`` are the caps of the kernels
(``zs_mix_max_dim()`` / ``zs_mix_max_components()``)."""
import ctypes
import os

import torch

from . import _binding, _hip

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libzs_mix.so")
ABI_VERSION = 1
MAX_DIM = 64
MAX_COMPONENTS = 65536
WS_PREP, WS_GRAD_PARAMS = 0, 1

_p = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64

_PROTOTYPES = _binding.both({
    # logits, mean, logstd, prep, C, D, stream
    "zs_mix_prepare": [_p, _p, _p, _p, _i64, _i64, _p],
    # x, prep, lp, R, C, D, stream
    "zs_mix_logprob": [_p, _p, _p, _i64, _i64, _i64, _p],
    # x, g, lp, prep, dx, R, C, D, stream
    "zs_mix_grad_x": [_p, _p, _p, _p, _p, _i64, _i64, _i64, _p],
    # x, g, lp, mean, logstd, prep, part, dlogits, dmean, dlogstd, R, C, D, shares, stream
    "zs_mix_grad_params": [_p, _p, _p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _p],
})
_PROTOTYPES["zs_mix_max_dim"] = (_i, [])
_PROTOTYPES["zs_mix_max_components"] = (_i, [])
_PROTOTYPES["zs_mix_panels"] = (_i64, [_i, _i64])                              # elem_bytes, C
_PROTOTYPES["zs_mix_row_shares"] = (_i64, [_i, _i64, _i64])                    # elem_bytes, R, C
_PROTOTYPES["zs_mix_workspace_elems"] = (_i64, [_i, _i, _i64, _i64, _i64])     # which, elem_bytes, C, D, shares

_LIB = None


def MixLibrary(path):
    """A freshly loaded, uncached ``_binding.Library`` of the zs_mix_* C ABI from the file at ``path``; ``lib()`` keeps the
    in-tree one."""
    from .distributions import _mix_functions
    library = _binding.Library(path, who="zhusuan.distributions (normal mixture)", make_target="mix",
                               abi_symbol="zs_mix_abi_version", abi_version=ABI_VERSION, prototypes=_PROTOTYPES)
    caps = (library.raw("zs_mix_max_dim"), library.raw("zs_mix_max_components"))
    if not caps == (MAX_DIM, MAX_COMPONENTS) == (_mix_functions.MAX_DIM, _mix_functions.MAX_COMPONENTS):
        raise RuntimeError("%s takes (D, C) up to %s, zhusuan._mix_hip states %s and the distribution routes by %s: the three must "
                           "agree" % (path, caps, (MAX_DIM, MAX_COMPONENTS), (_mix_functions.MAX_DIM, _mix_functions.MAX_COMPONENTS)))
    return library


def lib(path=None):
    """The mixture-of-Gaussians library (lazy); ``path`` loads another file instead of the in-tree one and does not replace it."""
    return _binding.lazy_lib(globals(), MixLibrary, path)


def _sfx(dtype):
    return _binding.suffix(dtype, "zhusuan.distributions (normal mixture): the parameters must be float32 or float64, got %s")


def workspace(which, ref, C, D, shares=1):
    """An uninitialised workspace of the size ``zs_mix_workspace_elems`` states, like ``ref``."""
    n = lib().raw("zs_mix_workspace_elems", which, ref.element_size(), C, D, shares)
    if n < 0:
        raise RuntimeError("zs_mix_workspace_elems rejected (which=%d, C=%d, D=%d, shares=%d)" % (which, C, D, shares))
    return torch.empty(n, dtype=ref.dtype, device=ref.device)


def _call(name, ref, operands, *args):
    _hip.require_device(ref, *operands)
    lib().call(name + _sfx(ref.dtype), *args, _hip.stream_for(ref))


def logprob(logits, mean, logstd, x):
    """(lp [R], prep): the prologue and the forward; ``prep`` (the centre, log_softmax, b, the packed operand) serves the
    backwards of the same parameters."""
    (C, D), R = mean.shape, x.shape[0]
    prep = workspace(WS_PREP, mean, C, D)
    lp = torch.empty(R, dtype=mean.dtype, device=mean.device)
    _call("zs_mix_prepare", mean, [logits, logstd], _hip.ptr(logits), _hip.ptr(mean), _hip.ptr(logstd), _hip.ptr(prep), C, D)
    _call("zs_mix_logprob", mean, [x, prep], _hip.ptr(x), _hip.ptr(prep), _hip.ptr(lp), R, C, D)
    return lp, prep


def grad_x(mean, x, g, lp, prep):
    """dx [R, D] (one launch, no workspace)."""
    (C, D), R = mean.shape, x.shape[0]
    dx = torch.empty_like(x)
    _call("zs_mix_grad_x", mean, [x, g, lp, prep], _hip.ptr(x), _hip.ptr(g), _hip.ptr(lp), _hip.ptr(prep), _hip.ptr(dx), R, C, D)
    return dx


def grad_params(logits, mean, logstd, x, g, lp, prep):
    """(dlogits [C], dmean [C, D], dlogstd [C, D], part) (two launches); the partials are ``[shares, K16 + 1, Cpad]``."""
    (C, D), R = mean.shape, x.shape[0]
    shares = max(int(lib().raw("zs_mix_row_shares", mean.element_size(), R, C)), 1)
    part = workspace(WS_GRAD_PARAMS, mean, C, D, shares)
    dlogits, dmean, dlogstd = torch.empty_like(logits), torch.empty_like(mean), torch.empty_like(logstd)
    _call("zs_mix_grad_params", mean, [x, g, lp, logstd, prep], _hip.ptr(x), _hip.ptr(g), _hip.ptr(lp), _hip.ptr(mean), _hip.ptr(logstd),
          _hip.ptr(prep), _hip.ptr(part), _hip.ptr(dlogits), _hip.ptr(dmean), _hip.ptr(dlogstd), R, C, D, shares)
    return dlogits, dmean, dlogstd, part
