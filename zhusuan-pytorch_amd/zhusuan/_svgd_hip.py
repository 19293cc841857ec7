"""ctypes binding of the Stein-variational-gradient-descent library (C ABI: include/zs_svgd.h).

A library of its own, ``zhusuan-pytorch_amd/lib/libzs_svgd.so`` (``make -C zhusuan-pytorch_amd/csrc svgd``, run by
``__graft_entry__.build()``), loaded on the first SVGD step on a HIP device: ``import zhusuan`` imports neither this module nor
the library.  There is no fallback here: a missing library, or a tensor that is not resident on a HIP device, raises.

``zhusuan.mcmc.SVGD`` goes through ``gram()``, ``finish()`` and ``update()`` below, looked up on this module at call time.  The
latents of a call are a list of at most MAX_TENSORS contiguous tensors of one dtype whose leading axis (or axes, flattened) is
the K particles."""
import ctypes
import os

from . import _binding, _hip

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libzs_svgd.so")
ABI_VERSION = 1
MAX_TENSORS = 32                    # ZS_SVGD_MAX_TENSORS
MAX_PARTICLES = {4: 256, 8: 128}    # zs_svgd_max_particles_of(element size)
SLAB = 32                           # ZS_SVGD_SLAB
GRID_CAP = 128                      # ZS_SVGD_GRID_CAP
STATE_HEADER = 4                    # ZS_SVGD_STATE_HEADER: h, 2 / h, med, K; then s [K], then k [K, K]

_p = ctypes.c_void_p
_d = ctypes.c_double
_i = ctypes.c_int
_i64 = ctypes.c_int64


class SvgdTensor(ctypes.Structure):          # struct zs_svgd_tensor
    _fields_ = [("q_in", _p), ("grad", _p), ("q_out", _p), ("h", _p), ("start", _i64), ("row", _i64)]


_PROTOTYPES = _binding.both({
    "zs_svgd_gram": [_p, _i, _i64, _i64, _p, _p],                                # tensors, n_tensors, n, K, partials, stream
    # tensors, n_tensors, n, K, state, step_size, adagrad, first, alpha, fudge, stream
    "zs_svgd_update": [_p, _i, _i64, _i64, _p, _d, _i, _i, _d, _d, _p],
})
_PROTOTYPES["zs_svgd_finish"] = [_p, _i64, _i64, _i, _d, _p, _p]                 # partials, n_slots, K, median, bandwidth, state, stream
_PROTOTYPES["zs_svgd_max_particles"] = (_i, [])
_PROTOTYPES["zs_svgd_max_particles_of"] = (_i, [_i])
_PROTOTYPES["zs_svgd_slab"] = (_i, [])
_PROTOTYPES["zs_svgd_grid_cap"] = (_i, [])
_PROTOTYPES["zs_svgd_gram_slots"] = (_i64, [_i64])
_PROTOTYPES["zs_svgd_partial_doubles"] = (_i64, [_i64])
_PROTOTYPES["zs_svgd_state_doubles"] = (_i64, [_i64])

_LIB = None


def SvgdLibrary(path):
    """A freshly loaded, uncached ``_binding.Library`` of the zs_svgd_* C ABI from the file at ``path``; ``lib()`` keeps the
    in-tree one."""
    library = _binding.Library(path, who="zhusuan.mcmc.SVGD", make_target="svgd", abi_symbol="zs_svgd_abi_version",
                               abi_version=ABI_VERSION, prototypes=_PROTOTYPES)
    got = ({nb: library.raw("zs_svgd_max_particles_of", nb) for nb in (4, 8)}, library.raw("zs_svgd_slab"),
           library.raw("zs_svgd_grid_cap"))
    if got != (MAX_PARTICLES, SLAB, GRID_CAP):
        raise RuntimeError("%s has (particle caps, slab, grid cap) = %s, zhusuan._svgd_hip routes by %s: the two must agree"
                           % (path, got, (MAX_PARTICLES, SLAB, GRID_CAP)))
    return library


def lib(path=None):
    """The SVGD library (lazy); ``path`` loads another file instead of the in-tree one and does not replace it."""
    return _binding.lazy_lib(globals(), SvgdLibrary, path)


def _sfx(dtype):
    return _binding.suffix(dtype, "zhusuan.mcmc.SVGD: latents must be float32 or float64, got %s")


def slots(n_columns):
    """Partials that ``gram`` writes for a table of ``n_columns`` columns (zs_svgd_gram_slots)."""
    return min((int(n_columns) + SLAB - 1) // SLAB, GRID_CAP)


def state_doubles(K):
    return STATE_HEADER + K + K * K


def _table(K, columns, ref):
    return _binding.flat_table(SvgdTensor, columns, ref, "zhusuan.mcmc.SVGD", K)


def gram(K, q, partials, library=None):
    """S1 over the tensors of ``q``: writes ``slots(columns)`` partials, float64 [K, K] each, at the start of ``partials``."""
    table, n, every = _table(K, dict(q_in=q), q)
    _hip.require_device(*(every + [partials]))
    (library or lib()).call("zs_svgd_gram" + _sfx(q[0].dtype), table, len(q), n, int(K), _hip.ptr(partials), _hip.stream_for(q[0]))


def finish(K, partials, n_slots, state, bandwidth=None, library=None):
    """S2: the first ``n_slots`` partials -> the state block (float64 [state_doubles(K)]); ``bandwidth`` None is the median rule."""
    _hip.require_device(partials, state)
    (library or lib()).call("zs_svgd_finish", _hip.ptr(partials), int(n_slots), int(K), int(bandwidth is None),
                            0.0 if bandwidth is None else float(bandwidth), _hip.ptr(state), _hip.stream_for(state))


def update(K, q_in, grad, q_out, state, step_size, h=None, first=True, alpha=0.9, fudge=1e-6, library=None):
    """S3 over the tensors of ``q_in``; ``h`` (a list like ``q_in``) switches the AdaGrad preconditioner on."""
    table, n, every = _table(K, dict(q_in=q_in, grad=grad, q_out=q_out, h=h), q_in)
    _hip.require_device(*(every + [state]))
    (library or lib()).call("zs_svgd_update" + _sfx(q_in[0].dtype), table, len(q_in), n, int(K), _hip.ptr(state), float(step_size),
                            int(h is not None), int(bool(first)), float(alpha), float(fudge), _hip.stream_for(q_in[0]))
