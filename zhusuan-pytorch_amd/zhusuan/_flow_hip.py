"""ctypes binding of the normalising-flow kernel library (C ABI: include/zs_flow.h).

A library of its own, ``zhusuan-pytorch_amd/lib/libzs_flow.so`` (``make -C zhusuan-pytorch_amd/csrc flow``, run by
``__graft_entry__.build()``), loaded on the first flow kernel call: ``import zhusuan`` and the variational and sampler
paths do not need it.  There is no fallback: a missing library, or a tensor that is not resident on a HIP device, raises.

Every kernel call of ``zhusuan.invertible`` and of ``FlowDistribution`` goes through the module-level functions below
(``split`` ... ``tail_bwd``), looked up on this module at call time.  Each is exactly one launch and allocates nothing:
the caller hands in contiguous operands and the outputs to fill.
"""
import ctypes
import os

from . import _binding, _hip

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libzs_flow.so")
ABI_VERSION = 1

MASK, INTERLEAVE = 0, 1
NORMAL, LOGISTIC = 0, 1
LOGDET_NONE, LOGDET_SCALAR, LOGDET_ROWS = 0, 1, 2

_p = ctypes.c_void_p
_d = ctypes.c_double
_i = ctypes.c_int
_n = ctypes.c_int64

# name -> argument types (without the _f32 / _f64 suffix), in the order of include/zs_flow.h
_PROTOTYPES = _binding.both({
    "zs_flow_split": [_i, _p, _p, _p, _n, _n, _i, _p],
    "zs_flow_split_bwd": [_i, _p, _p, _p, _n, _n, _i, _p],
    "zs_flow_merge": [_i, _p, _p, _p, _d, _p, _n, _n, _i, _p],
    "zs_flow_merge_bwd": [_i, _p, _p, _d, _p, _p, _n, _n, _i, _p],
    "zs_flow_scale_fwd": [_p, _p, _d, _p, _p, _n, _n, _p],
    "zs_flow_scale_bwd": [_p, _p, _p, _p, _d, _p, _p, _n, _n, _p],
    "zs_flow_made_fwd": [_p, _p, _p, _p, _n, _n, _p],
    "zs_flow_made_bwd": [_p, _p, _p, _p, _p, _p, _n, _n, _p],
    "zs_flow_made_inv_col": [_p, _p, _p, _n, _n, _n, _p],
    "zs_flow_tail": [_i, _p, _p, _p, _i, _p, _i, _p, _n, _n, _p],
    "zs_flow_tail_bwd": [_i, _p, _p, _p, _p, _i, _p, _p, _n, _n, _p],
})

_LIB = None


def FlowLibrary(path):
    """A freshly loaded, uncached ``_binding.Library`` of the zs_flow_* C ABI from the file at ``path``; ``lib()`` keeps the
    in-tree one."""
    return _binding.Library(path, who="zhusuan.invertible", what="flow kernel library", make_target="flow",
                            abi_symbol="zs_flow_abi_version", abi_version=ABI_VERSION, prototypes=_PROTOTYPES)


def lib(path=None):
    """The flow library (lazy); ``path`` loads another file instead of the in-tree one and does not replace it."""
    return _binding.lazy_lib(globals(), FlowLibrary, path)


def _suffix(dtype):
    return _binding.suffix(dtype, "zhusuan.invertible: tensors must be float32 or float64, got %s")


def check_dtype(*tensors):
    """float32 or float64, one dtype for all (None entries are absent operands); returns it."""
    dt = None
    for t in tensors:
        if t is None:
            continue
        _suffix(t.dtype)
        if dt is None:
            dt = t.dtype
        elif t.dtype != dt:
            raise RuntimeError("zhusuan.invertible: operands of one kernel must share a dtype, got %s and %s" % (dt, t.dtype))
    return dt


def _call(base, first, tensors, *args):
    """``first``: the tensor that decides dtype and stream; ``tensors``: every operand (contiguity, dtype, device checked)."""
    dt = check_dtype(*tensors)
    for t in tensors:
        if t is not None and not t.is_contiguous():
            raise RuntimeError("zhusuan.invertible: kernel operands must be contiguous")
    _hip.require_device(*tensors)
    lib().call(base + _suffix(dt), *(args + (_hip.stream_for(first),)))


def _bd(t):
    if t.dim() != 2:
        raise RuntimeError("zhusuan.invertible: expected a [B, D] tensor, got shape %s" % (tuple(t.shape),))
    return int(t.shape[0]), int(t.shape[1])


def split(mode, x, mask, out, sel=0):
    """MASK: out = mask * x.  INTERLEAVE: out[b, j] = x[b, 2j + sel] (out is [B, D/2])."""
    B, D = _bd(x)
    _call("zs_flow_split", x, (x, mask, out), int(mode), _hip.ptr(x), _hip.ptr(mask), _hip.ptr(out), B, D, int(sel))


def split_bwd(mode, g_out, mask, gx, sel=0):
    """MASK: gx = mask * g_out.  INTERLEAVE: gx[b, 2j + sel] = g_out[b, j], zero at 2j + 1 - sel (gx is [B, D])."""
    B, D = _bd(gx)
    _call("zs_flow_split_bwd", gx, (g_out, mask, gx), int(mode), _hip.ptr(g_out), _hip.ptr(mask), _hip.ptr(gx), B, D, int(sel))


def merge(mode, x, mask, shift, sign, y, sel=0):
    """MASK: y = mask*x + ((1-mask)*x + (sign*shift)*(1-mask)).  INTERLEAVE: y[b, 2j+1-sel] = x[b, 2j+1-sel] + sign*shift[b, j]."""
    B, D = _bd(x)
    _call("zs_flow_merge", x, (x, mask, shift, y), int(mode), _hip.ptr(x), _hip.ptr(mask), _hip.ptr(shift), float(sign),
          _hip.ptr(y), B, D, int(sel))


def merge_bwd(mode, gy, mask, sign, gx, gshift, sel=0):
    """gx and gshift of ``merge`` from one read of gy."""
    B, D = _bd(gy)
    _call("zs_flow_merge_bwd", gy, (gy, mask, gx, gshift), int(mode), _hip.ptr(gy), _hip.ptr(mask), float(sign), _hip.ptr(gx),
          _hip.ptr(gshift), B, D, int(sel))


def scale_fwd(x, log_scale, sign, y, logdet):
    """y = x * exp(sign * log_scale) (y may be x) and logdet[()] = sum(log_scale), one launch."""
    B, D = _bd(x)
    _call("zs_flow_scale_fwd", x, (x, log_scale, y, logdet), _hip.ptr(x), _hip.ptr(log_scale), float(sign), _hip.ptr(y),
          _hip.ptr(logdet), B, D)


def scale_bwd(gy, y, log_scale, g_logdet, sign, gx, g_log_scale):
    """gx = gy * exp(sign * log_scale); g_log_scale[d] = sign * sum_b gy*y + g_logdet (None = 0), one launch."""
    B, D = _bd(gy)
    _call("zs_flow_scale_bwd", gy, (gy, y, log_scale, g_logdet, gx, g_log_scale), _hip.ptr(gy), _hip.ptr(y), _hip.ptr(log_scale),
          _hip.ptr(g_logdet), float(sign), _hip.ptr(gx), _hip.ptr(g_log_scale), B, D)


def made_fwd(x, net, u, logdet):
    """u = (x - m) * exp(-loga), logdet = -loga, with (m, loga) the halves of net [B, 2D] read in place."""
    B, D = _bd(x)
    _call("zs_flow_made_fwd", x, (x, net, u, logdet), _hip.ptr(x), _hip.ptr(net), _hip.ptr(u), _hip.ptr(logdet), B, D)


def made_bwd(gu, gld, x, net, gx, gnet):
    """gx and the [B, 2D] gradient of net from gu / gld (either may be None)."""
    B, D = _bd(x)
    _call("zs_flow_made_bwd", x, (gu, gld, x, net, gx, gnet), _hip.ptr(gu), _hip.ptr(gld), _hip.ptr(x), _hip.ptr(net),
          _hip.ptr(gx), _hip.ptr(gnet), B, D)


def made_inv_col(u, net, x, col):
    """x[:, col] = u[:, col] * exp(loga[:, col]) + m[:, col]."""
    B, D = _bd(u)
    _call("zs_flow_made_inv_col", u, (u, net, x), _hip.ptr(u), _hip.ptr(net), _hip.ptr(x), B, D, int(col))


def tail(base, z, loc, scale, param_rows, logdet, logdet_kind, out):
    """out[b] = sum_d logpdf(z[b, d]; loc, scale) + logdet."""
    B, D = _bd(z)
    _call("zs_flow_tail", z, (z, loc, scale, logdet, out), int(base), _hip.ptr(z), _hip.ptr(loc), _hip.ptr(scale),
          int(param_rows), _hip.ptr(logdet), int(logdet_kind), _hip.ptr(out), B, D)


def tail_bwd(base, g, z, loc, scale, param_rows, gz, g_logdet):
    """gz[b, d] = g[b] * d logpdf / dz; g_logdet[b] = g[b] when g_logdet is given."""
    B, D = _bd(z)
    _call("zs_flow_tail_bwd", z, (g, z, loc, scale, gz, g_logdet), int(base), _hip.ptr(g), _hip.ptr(z), _hip.ptr(loc),
          _hip.ptr(scale), int(param_rows), _hip.ptr(gz), _hip.ptr(g_logdet), B, D)
