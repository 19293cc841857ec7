"""ctypes binding of the inclusive-KL library (C ABI: include/zs_klpq.h).

A library of its own, ``zhusuan-pytorch_amd/lib/libzs_klpq.so`` (``make -C zhusuan-pytorch_amd/csrc klpq``, run by
``__graft_entry__.build()``), loaded on the first kernel call of ``InclusiveKLObjective`` or ``is_loglikelihood``:
``import zhusuan`` and every other objective do not need it.  There is no fallback: a missing library, or a tensor that is not
resident on a HIP device, raises.

``zhusuan.variational._klpq_functions`` goes through ``forward`` and ``backward`` below, looked up on this module at call time.
A term is a 2-D tensor ``[K or 1, B or 1]`` of any strides: it is handed to the kernel by address and strides, never copied, and a
size-1 axis enters with stride 0 (the term is shared along it); the backward takes the terms' layouts (``layout``), not the
terms.  ``_binding.flat_table`` serves contiguous tensors of one size, so the table of strided terms is filled here.
``MAX_TERMS`` is the number of terms a side takes (``zs_klpq_max_terms()``),
``MEAN_MAX_BATCH`` the largest batch whose mean the launch forms itself (``zs_klpq_mean_max_batch()``)."""
import ctypes
import os

import torch

from . import _binding, _hip

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libzs_klpq.so")
ABI_VERSION = 1
MAX_TERMS = 8
MEAN_MAX_BATCH = 1024
MODEL_GRAD, BOUND_ONLY, GCOST_MEAN = 1, 2, 4

_p = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64


class KlpqTerm(ctypes.Structure):          # struct zs_klpq_term
    _fields_ = [("value", _p), ("grad", _p), ("sk", _i64), ("sb", _i64)]


_PROTOTYPES = _binding.both({
    # p, Tp, q, Tq, K, B, flags, w, cost, bound, ess, mean_cost, stream
    "zs_klpq_forward": [_p, _i, _p, _i, _i64, _i64, _i, _p, _p, _p, _p, _p, _p],
    # p, Tp, q, Tq, K, B, flags, w, gcost, gbound, stream
    "zs_klpq_backward": [_p, _i, _p, _i, _i64, _i64, _i, _p, _p, _p, _p],
})
_PROTOTYPES["zs_klpq_max_terms"] = (_i, [])
_PROTOTYPES["zs_klpq_mean_max_batch"] = (_i64, [])
_PROTOTYPES["zs_klpq_group_lanes"] = (_i, [_i64])          # K -> lanes per datapoint

_LIB = None


def KlpqLibrary(path):
    """A freshly loaded, uncached ``_binding.Library`` of the zs_klpq_* C ABI from the file at ``path``; ``lib()`` keeps the
    in-tree one."""
    return _binding.Library(path, who="zhusuan.variational (inclusive KL)", make_target="klpq",
                            abi_symbol="zs_klpq_abi_version", abi_version=ABI_VERSION, prototypes=_PROTOTYPES)


def lib(path=None):
    """The inclusive-KL library (lazy); ``path`` loads another file instead of the in-tree one and does not replace it."""
    return _binding.lazy_lib(globals(), KlpqLibrary, path)


def _sfx(dtype):
    return _binding.suffix(dtype, "zhusuan.variational (inclusive KL): log-probabilities must be float32 or float64, got %s")


def layout(t):
    """((K or 1, B or 1), (sk, sb)) of a 2-D term, strides in elements; a size-1 axis is shared (stride 0)."""
    (k, b), (sk, sb) = t.shape, t.stride()
    return (k, b), (0 if k == 1 else sk, 0 if b == 1 else sb)


def table(values=None, layouts=None, grads=None):
    """The host table of one side: a row per term with its strides and the address of its values (``values``: the tensors; their
    layouts are read off them) and / or of its gradient (``grads[i]``: a tensor laid out like the term, or None)."""
    if layouts is None:
        layouts = [layout(t) for t in values]
    tab = (KlpqTerm * max(len(layouts), 1))()
    for i, (_, (sk, sb)) in enumerate(layouts):
        row = tab[i]
        row.sk, row.sb = sk, sb
        if values is not None:
            row.value = values[i].data_ptr()
        if grads is not None and grads[i] is not None:
            row.grad = grads[i].data_ptr()
    return tab


def _check(terms_p, terms_q, K, B):
    ref = terms_q[0]
    for t in list(terms_p) + list(terms_q):
        if t.dim() != 2 or t.shape[0] not in (1, K) or t.shape[1] not in (1, B) or t.dtype != ref.dtype:
            raise RuntimeError("zhusuan.variational (inclusive KL): every term must be a [K or 1, B or 1] tensor of one dtype")
    return ref


def forward(terms_p, terms_q, K, B, model_grad=False, bound_only=False, want_mean=False):
    """Q1 in one launch: ``(w [B, K], cost [B], bound [B], ess [B], mean_cost [] or None)``; with ``bound_only`` everything but
    ``bound`` is None.  ``want_mean`` needs ``B <= MEAN_MAX_BATCH``."""
    ref = _check(terms_p, terms_q, K, B)
    _hip.require_device(*(list(terms_p) + list(terms_q)))

    def new(*shape):
        return torch.empty(shape, dtype=ref.dtype, device=ref.device)
    bound = new(B)
    w = cost = ess = mean = None
    if not bound_only:
        w, cost, ess = new(B, K), new(B), new(B)
        mean = new() if want_mean else None
    flags = (MODEL_GRAD if model_grad else 0) | (BOUND_ONLY if bound_only else 0)
    lib().call("zs_klpq_forward" + _sfx(ref.dtype), table(values=terms_p), len(terms_p), table(values=terms_q), len(terms_q), int(K), int(B), flags,
               _hip.ptr(w), _hip.ptr(cost), _hip.ptr(bound), _hip.ptr(ess), _hip.ptr(mean), _hip.stream_for(ref))
    return w, cost, bound, ess, mean


def backward(layouts_p, layouts_q, want_p, want_q, K, B, w, gcost, gbound=None, model_grad=False, gcost_is_mean=False):
    """The backward in one launch: (gradients of the generator terms, of the variational terms), each a fresh tensor with its
    term's shape and strides (``layouts_*``: what ``layout`` gave for the terms of the forward call; the kernel does not read
    their values again), or None where ``want_*[i]`` is false.  ``gcost``: ``[B]``, or one element with ``gcost_is_mean``."""
    _hip.require_device(w, gcost, gbound)

    def new(lay, want):
        if not want:
            return None
        (k, b), (sk, sb) = lay
        if (k not in (1, K)) or (b not in (1, B)) or sorted((abs(sk) or 1, abs(sb) or 1)) not in ([1, 1], [1, b], [1, k]):
            raise RuntimeError("zhusuan.variational (inclusive KL): a term must be dense ([K, B] or [B, K] order) to receive a gradient")
        return torch.empty_strided((k, b), (sk or 1, sb or 1), dtype=w.dtype, device=w.device)
    gp = [new(lay, want) for lay, want in zip(layouts_p, want_p)]
    gq = [new(lay, want) for lay, want in zip(layouts_q, want_q)]
    flags = (MODEL_GRAD if model_grad else 0) | (GCOST_MEAN if gcost_is_mean else 0)
    lib().call("zs_klpq_backward" + _sfx(w.dtype), table(layouts=layouts_p, grads=gp), len(layouts_p), table(layouts=layouts_q, grads=gq),
               len(layouts_q), int(K), int(B), flags, _hip.ptr(w), _hip.ptr(gcost), _hip.ptr(gbound), _hip.stream_for(w))
    return gp, gq
