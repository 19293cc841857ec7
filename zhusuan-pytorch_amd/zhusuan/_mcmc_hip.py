"""ctypes binding of the stochastic-gradient MCMC update library (C ABI: include/zs_mcmc.h).

A library of its own, ``zhusuan-pytorch_amd/lib/libzs_mcmc.so`` (``make -C zhusuan-pytorch_amd/csrc mcmc``, run by
``__graft_entry__.build()``), loaded on the first update: ``import zhusuan`` and the variational path do not need it.
There is no fallback: a missing library, or a tensor that is not resident on a HIP device, raises.

Every update of ``zhusuan.mcmc`` goes through ``update()`` below, looked up on this module at call time.
"""
import ctypes
import os

from . import _binding, _hip

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libzs_mcmc.so")
ABI_VERSION = 1
MAX_TENSORS = 32          # ZS_MCMC_MAX_TENSORS

SGLD, PSGLD, SGHMC_PRE, SGHMC_POST = 0, 1, 2, 3
SECOND_ORDER, RESAMPLE_V = 1, 2

_p = ctypes.c_void_p
_d = ctypes.c_double


class McmcTensor(ctypes.Structure):          # struct zs_mcmc_tensor
    _fields_ = [("q_in", _p), ("q_out", _p), ("grad", _p), ("state", _p), ("z", _p), ("start", ctypes.c_int64)]


_PROTOTYPES = _binding.both({
    "zs_mcmc_update": [ctypes.c_int, _p, ctypes.c_int, ctypes.c_int64, _d, _d, _d, _d, _d, ctypes.c_int, ctypes.c_uint64,
                       ctypes.c_uint64, _p, _p],
})

_LIB = None


def McmcLibrary(path):
    """A freshly loaded, uncached ``_binding.Library`` of the zs_mcmc_* C ABI from the file at ``path``; ``lib()`` keeps the
    in-tree one."""
    return _binding.Library(path, who="zhusuan.mcmc", what="sampler kernel library", make_target="mcmc",
                            abi_symbol="zs_mcmc_abi_version", abi_version=ABI_VERSION, prototypes=_PROTOTYPES)


def lib(path=None):
    """The sampler library (lazy); ``path`` loads another file instead of the in-tree one and does not replace it."""
    return _binding.lazy_lib(globals(), McmcLibrary, path)


def update(kind, q_in, q_out, grad=None, state=None, z=None, lr=0., decay=0., epsilon=0., alpha=0., beta=0., flags=0,
           seed=0, call=0, rng_state=None, library=None):
    """One launch of the fused update over the tensors of ``q_in`` (a list of at most MAX_TENSORS contiguous tensors of one
    dtype on one HIP device).  ``q_out``: where the updated values go (may be the same tensors); ``grad`` / ``state``:
    lists like ``q_in`` or None where the kind does not read them; ``z``: None, or a list whose entries are injected
    standard normals or None (drawn in-kernel from Philox (seed, call), or from ``rng_state`` + call).  The flat index space
    of the launch is the tensors in list order."""
    table, n, every = _binding.flat_table(McmcTensor, dict(q_in=q_in, q_out=q_out, grad=grad, state=state, z=z), q_in,
                                          "zhusuan.mcmc")
    if not q_in:
        return
    _hip.require_device(*(every + [rng_state]))
    sfx = _binding.suffix(q_in[0].dtype, "zhusuan.mcmc: latents must be float32 or float64, got %s")
    (library or lib()).call("zs_mcmc_update" + sfx, int(kind), table, len(q_in), n, float(lr), float(decay), float(epsilon),
                            float(alpha), float(beta), int(flags), _binding.u64(seed), _binding.u64(call),
                            _hip.ptr(rng_state), _hip.stream_for(q_in[0]))
