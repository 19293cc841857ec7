"""ctypes binding of the admixture-likelihood library (C ABI: include/zs_topic.h).

A library of its own, ``zhusuan-pytorch_amd/lib/libzs_topic.so`` (``make -C zhusuan-pytorch_amd/csrc topic``, run by
``__graft_entry__.build()``), loaded on the first kernel call of ``AdmixtureMultinomial``: ``import zhusuan`` imports neither
this module nor the library.  There is no fallback here: a missing library, or a tensor that is not resident on a HIP device,
raises.

``zhusuan.distributions._topic_functions`` goes through the functions below, looked up on this module at call time.  They take
contiguous tensors -- ``H [R, K]``, ``B [K, V]``, ``X [Dx, V]``, ``g [R]`` --, allocate the outputs and the workspaces the ABI
asks for, and return them.  ``MAX_TOPICS`` is the most topics the kernels take (``zs_topic_max_topics()``)."""
import ctypes
import os

import torch

from . import _binding, _hip

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libzs_topic.so")
ABI_VERSION = 1
MAX_TOPICS = 128
WS_PREP, WS_LOGPROB, WS_GRAD_DOC, WS_GRAD_TOPIC = 0, 1, 2, 3

_p = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64

_PROTOTYPES = _binding.both({
    # H, B, X, prep, R, K, V, Dx, stream
    "zs_topic_prepare": [_p, _p, _p, _p, _i64, _i64, _i64, _i64, _p],
    # B, X, prep, part, lp, R, K, V, Dx, stream
    "zs_topic_logprob": [_p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _p],
    # B, X, g, prep, part, dH, R, K, V, Dx, splits, stream
    "zs_topic_grad_doc": [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _i64, _p],
    # B, X, g, prep, part, dB, R, K, V, Dx, stream
    "zs_topic_grad_topic": [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _i64, _p],
})
_PROTOTYPES["zs_topic_max_topics"] = (_i, [])
_PROTOTYPES["zs_topic_panels"] = (_i64, [_i, _i64])                                      # elem_bytes, V
_PROTOTYPES["zs_topic_doc_splits"] = (_i64, [_i, _i64, _i64])                            # elem_bytes, R, V
_PROTOTYPES["zs_topic_workspace_elems"] = (_i64, [_i, _i, _i64, _i64, _i64, _i64, _i64])   # which, elem_bytes, R, K, V, Dx, splits

_LIB = None


def TopicLibrary(path):
    """A freshly loaded, uncached ``_binding.Library`` of the zs_topic_* C ABI from the file at ``path``; ``lib()`` keeps the
    in-tree one."""
    from .distributions import _topic_functions
    library = _binding.Library(path, who="zhusuan.distributions (admixture multinomial)", make_target="topic",
                               abi_symbol="zs_topic_abi_version", abi_version=ABI_VERSION, prototypes=_PROTOTYPES)
    cap = library.raw("zs_topic_max_topics")
    if not cap == MAX_TOPICS == _topic_functions.MAX_TOPICS:
        raise RuntimeError("%s takes %d topics, zhusuan._topic_hip.MAX_TOPICS is %d and the distribution routes by %d: the three "
                           "must agree" % (path, cap, MAX_TOPICS, _topic_functions.MAX_TOPICS))
    return library


def lib(path=None):
    """The admixture-likelihood library (lazy); ``path`` loads another file instead of the in-tree one and does not replace it."""
    return _binding.lazy_lib(globals(), TopicLibrary, path)


def _sfx(dtype):
    return _binding.suffix(dtype, "zhusuan.distributions (admixture multinomial): logits must be float32 or float64, got %s")


def _shape(H, B, X):
    (R, K), V, Dx = H.shape, B.shape[1], X.shape[0]
    return int(R), int(K), int(V), int(Dx)


def workspace(which, ref, R, K, V, Dx, splits=1):
    """An uninitialised workspace of the size ``zs_topic_workspace_elems`` states, like ``ref``."""
    n = lib().raw("zs_topic_workspace_elems", which, ref.element_size(), R, K, V, Dx, splits)
    if n < 0:
        raise RuntimeError("zs_topic_workspace_elems rejected (which=%d, R=%d, K=%d, V=%d, Dx=%d, splits=%d)" % (which, R, K, V, Dx, splits))
    return torch.empty(n, dtype=ref.dtype, device=ref.device)


def _call(name, ref, operands, *args):
    _hip.require_device(ref, *operands)
    lib().call(name + _sfx(ref.dtype), *args, _hip.stream_for(ref))


def logprob(H, B, X):
    """(lp [R], prep): the prologue and the forward; ``prep`` (lse, N, Z, log Z, E) serves the backwards of the same operands."""
    R, K, V, Dx = _shape(H, B, X)
    prep = workspace(WS_PREP, H, R, K, V, Dx)
    part = workspace(WS_LOGPROB, H, R, K, V, Dx)
    lp = torch.empty(R, dtype=H.dtype, device=H.device)
    _call("zs_topic_prepare", H, [B, X], _hip.ptr(H), _hip.ptr(B), _hip.ptr(X), _hip.ptr(prep), R, K, V, Dx)
    _call("zs_topic_logprob", H, [B, X], _hip.ptr(B), _hip.ptr(X), _hip.ptr(prep), _hip.ptr(part), _hip.ptr(lp), R, K, V, Dx)
    return lp, prep


def grad_doc(H, B, X, g, prep):
    """dH [R, K] (two launches); the partials are ``[splits, R, K16]``."""
    R, K, V, Dx = _shape(H, B, X)
    splits = max(int(lib().raw("zs_topic_doc_splits", H.element_size(), R, V)), 1)
    part = workspace(WS_GRAD_DOC, H, R, K, V, Dx, splits)
    dH = torch.empty_like(H)
    _call("zs_topic_grad_doc", H, [B, X, g, prep], _hip.ptr(B), _hip.ptr(X), _hip.ptr(g), _hip.ptr(prep), _hip.ptr(part),
          _hip.ptr(dH), R, K, V, Dx, splits)
    return dH, part


def grad_topic(H, B, X, g, prep):
    """dB [K, V] (two launches); the partials are ``[panels, K16]``."""
    R, K, V, Dx = _shape(H, B, X)
    part = workspace(WS_GRAD_TOPIC, H, R, K, V, Dx)
    dB = torch.empty_like(B)
    _call("zs_topic_grad_topic", H, [B, X, g, prep], _hip.ptr(B), _hip.ptr(X), _hip.ptr(g), _hip.ptr(prep), _hip.ptr(part),
          _hip.ptr(dB), R, K, V, Dx)
    return dB, part
