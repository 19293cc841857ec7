"""ctypes binding of the planar / Householder flow library (C ABI: include/zs_nf.h).

A library of its own, ``zhusuan-pytorch_amd/lib/libzs_nf.so`` (``make -C zhusuan-pytorch_amd/csrc nf``, run by
``__graft_entry__.build()``), loaded on the first kernel call of ``zhusuan.transform``: ``import zhusuan`` does not need it.
There is no fallback: a missing library, or a tensor that is not resident on a HIP device, raises.

``zhusuan.transform._functions`` goes through the functions below, looked up on this module at call time.  They take contiguous
tensors -- ``u``, ``w`` as ``[L, D]``, ``b`` as ``[L]``, rows as ``[R, D]``, ``v`` as ``[L, R, D]`` -- with ``L <= MAX_LAYERS`` and
``D <= MAX_DIM``, allocate the outputs and return them."""
import ctypes
import os

import torch

from . import _binding, _hip

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libzs_nf.so")
ABI_VERSION = 1
MAX_DIM = 64
MAX_LAYERS = 32

_p = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64

_PROTOTYPES = _binding.both({
    # u, w, b, x, y, logdet, R, D, L, stream
    "zs_nf_planar_fwd": [_p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _p],
    # u, w, b, x, gy, gld, gx, partials, R, D, L, stream
    "zs_nf_planar_bwd": [_p, _p, _p, _p, _p, _p, _p, _p, _i64, _i64, _i64, _p],
    # u, w, partials, n_wg, gu, gw, gb, D, L, stream
    "zs_nf_planar_finish": [_p, _p, _p, _i64, _p, _p, _p, _i64, _i64, _p],
    # v, x, y, R, D, L, stream
    "zs_nf_householder_fwd": [_p, _p, _p, _i64, _i64, _i64, _p],
    # v, x, gy, gx, gv, R, D, L, stream
    "zs_nf_householder_bwd": [_p, _p, _p, _p, _p, _i64, _i64, _i64, _p],
})
_PROTOTYPES["zs_nf_max_dim"] = (_i, [])
_PROTOTYPES["zs_nf_max_layers"] = (_i, [])
_PROTOTYPES["zs_nf_max_workgroups"] = (_i, [])
_PROTOTYPES["zs_nf_group_lanes"] = (_i, [_i64])                    # D -> lanes per row
_PROTOTYPES["zs_nf_planar_workgroups"] = (_i, [_i64, _i64])        # R, D -> leading extent of the partials

_LIB = None


def NfLibrary(path):
    """A freshly loaded, uncached ``_binding.Library`` of the zs_nf_* C ABI from the file at ``path``; ``lib()`` keeps the
    in-tree one."""
    return _binding.Library(path, who="zhusuan.transform (planar / Householder flows)", make_target="nf",
                            abi_symbol="zs_nf_abi_version", abi_version=ABI_VERSION, prototypes=_PROTOTYPES)


def lib(path=None):
    """The flow-stack library (lazy); ``path`` loads another file instead of the in-tree one and does not replace it."""
    return _binding.lazy_lib(globals(), NfLibrary, path)


def _sfx(dtype):
    return _binding.suffix(dtype, "zhusuan.transform: rows must be float32 or float64, got %s")


def _call(name, ref, operands, *args):
    _hip.require_device(ref, *operands)
    lib().call(name + _sfx(ref.dtype), *args, _hip.stream_for(ref))


def _new(ref, shape, want=True):
    return torch.empty(shape, dtype=ref.dtype, device=ref.device) if want else None


def planar_fwd(u, w, b, x, want_y=True, want_logdet=True):
    """P1: (y [R, D] or None, logdet [R] or None) of the L-layer planar stack in one launch."""
    (L, D), R = u.shape, x.shape[0]
    y, logdet = _new(x, (R, D), want_y), _new(x, (R,), want_logdet)
    _call("zs_nf_planar_fwd", x, [u, w, b], _hip.ptr(u), _hip.ptr(w), _hip.ptr(b), _hip.ptr(x), _hip.ptr(y), _hip.ptr(logdet),
          R, D, L)
    return y, logdet


def planar_bwd(u, w, b, x, gy=None, gld=None, want_gx=True, want_partials=True):
    """P1b: (gx [R, D] or None, partials [n_wg, L, 2 D + 2] or None) from the cotangents gy [R, D] / gld [R] (None = zero)."""
    (L, D), R = u.shape, x.shape[0]
    gx = _new(x, (R, D), want_gx)
    partials = None
    if want_partials:
        _hip.require_device(x)
        partials = _new(x, (lib().raw("zs_nf_planar_workgroups", R, D), L, 2 * D + 2))
    _call("zs_nf_planar_bwd", x, [u, w, b, gy, gld], _hip.ptr(u), _hip.ptr(w), _hip.ptr(b), _hip.ptr(x), _hip.ptr(gy),
          _hip.ptr(gld), _hip.ptr(gx), _hip.ptr(partials), R, D, L)
    return gx, partials


def planar_finish(u, w, partials, want_gu=True, want_gw=True, want_gb=True):
    """P1f: (gu [L, D], gw [L, D], gb [L]; None where not wanted) from the partials of ``planar_bwd``."""
    L, D = u.shape
    if partials.shape[0] == 0:          # no rows: nothing was summed
        return tuple(torch.zeros(s, dtype=u.dtype, device=u.device) if want else None
                     for s, want in (((L, D), want_gu), ((L, D), want_gw), ((L,), want_gb)))
    gu, gw, gb = _new(u, (L, D), want_gu), _new(u, (L, D), want_gw), _new(u, (L,), want_gb)
    _call("zs_nf_planar_finish", u, [w, partials], _hip.ptr(u), _hip.ptr(w), _hip.ptr(partials), partials.shape[0], _hip.ptr(gu),
          _hip.ptr(gw), _hip.ptr(gb), D, L)
    return gu, gw, gb


def householder_fwd(v, x):
    """H1: y [R, D] after the L reflections v [L, R, D], one launch."""
    L, R, D = v.shape
    y = _new(x, (R, D))
    _call("zs_nf_householder_fwd", x, [v], _hip.ptr(v), _hip.ptr(x), _hip.ptr(y), R, D, L)
    return y


def householder_bwd(v, x, gy, want_gx=True, want_gv=True):
    """H1b: (gx [R, D] or None, gv [L, R, D] or None)."""
    L, R, D = v.shape
    gx, gv = _new(x, (R, D), want_gx), _new(x, (L, R, D), want_gv)
    _call("zs_nf_householder_bwd", x, [v, gy], _hip.ptr(v), _hip.ptr(x), _hip.ptr(gy), _hip.ptr(gx), _hip.ptr(gv), R, D, L)
    return gx, gv
