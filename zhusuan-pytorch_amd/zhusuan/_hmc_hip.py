"""ctypes binding of the Hamiltonian Monte Carlo library (C ABI: include/zs_hmc.h).

A library of its own, ``zhusuan-pytorch_amd/lib/libzs_hmc.so`` (``make -C zhusuan-pytorch_amd/csrc hmc``, run by
``__graft_entry__.build()``), loaded on the first HMC iteration: ``import zhusuan``, the variational path and the
stochastic-gradient samplers do not need it.  There is no fallback: a missing library, or a tensor that is not resident on a
HIP device, raises.

``zhusuan.mcmc.HMC`` goes through ``move()``, ``decide()`` and ``select()`` below, looked up on this module at call time.
"""
import ctypes
import os

import torch

from . import _binding, _hip

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), "lib", "libzs_hmc.so")
ABI_VERSION = 1
MAX_TENSORS = 32          # ZS_HMC_MAX_TENSORS
MAX_CHUNKS = 16           # ZS_HMC_MAX_CHUNKS
TILE = 1024               # ZS_HMC_TILE
STATE_DOUBLES = 8         # ZS_HMC_STATE_DOUBLES

BEGIN, STEP, END = 0, 1, 2
# the state block
EPS, EPS_INIT, M, HBAR, LOG_EPS, LOG_EPSBAR, ABAR, NACC = range(8)

_p = ctypes.c_void_p
_d = ctypes.c_double
_i64 = ctypes.c_int64
_u64 = ctypes.c_uint64


class HmcTensor(ctypes.Structure):          # struct zs_hmc_tensor
    _fields_ = [("q0", _p), ("q", _p), ("p", _p), ("grad", _p), ("z", _p), ("p0", _p), ("q_out", _p), ("start", _i64), ("row", _i64)]


class HmcChunk(ctypes.Structure):           # struct zs_hmc_chunk
    _fields_ = [("k0", _p), ("k1", _p), ("slots", _i64), ("is_f64", ctypes.c_int32), ("pad", ctypes.c_int32)]


_PROTOTYPES = _binding.both({
    "zs_hmc_move": [ctypes.c_int, _p, ctypes.c_int, _i64, _i64, _p, _p, _u64, _u64, _p, _p],
    "zs_hmc_decide": [_p, ctypes.c_int, _i64, _p, _p, _p, _p, _p, _p, ctypes.c_int, _d, _d, _d, _d, _u64, _u64, _p, _p],
    "zs_hmc_select": [_p, ctypes.c_int, _i64, _i64, _p, _p],
})
_PROTOTYPES["zs_hmc_ksum_slots"] = (_i64, [_p, ctypes.c_int])          # rows (host array), n_tensors -> slots per chain, -1

_LIB = None


def HmcLibrary(path):
    """A freshly loaded, uncached ``_binding.Library`` of the zs_hmc_* C ABI from the file at ``path``; ``lib()`` keeps the
    in-tree one."""
    return _binding.Library(path, who="zhusuan.mcmc.HMC", make_target="hmc", abi_symbol="zs_hmc_abi_version",
                            abi_version=ABI_VERSION, prototypes=_PROTOTYPES)


def lib(path=None):
    """The HMC library (lazy); ``path`` loads another file instead of the in-tree one and does not replace it."""
    return _binding.lazy_lib(globals(), HmcLibrary, path)


def _sfx(dtype):
    return _binding.suffix(dtype, "zhusuan.mcmc.HMC: latents and log joints must be float32 or float64, got %s")


def pieces(row):
    """Slots of the kinetic workspace per chain for a tensor with `row` elements per chain (include/zs_hmc.h)."""
    return (int(row) + TILE - 2) // TILE + 1


def ksum_slots(rows):
    return sum(pieces(r) for r in rows)


def _table(n_chains, columns, ref):
    """The host table of a move / select: ``columns`` maps a field name to a list of tensors (or None entries) like ``ref``."""
    return _binding.flat_table(HmcTensor, columns, ref, "zhusuan.mcmc.HMC", n_chains)


def move(kind, n_chains, state, q, p, grad, q0=None, z=None, p0=None, ksum=None, seed=0, call=0, rng_state=None, library=None):
    """One launch of kind BEGIN / STEP / END over the tensors of ``q`` (a list of at most MAX_TENSORS contiguous tensors of one
    dtype on one HIP device, each with ``n_chains`` leading rows).  ``state``: the device-resident step-size block (float64[8]);
    ``ksum``: the kinetic workspace (BEGIN, END), ``n_chains * ksum_slots(rows)`` elements of the latents' dtype."""
    if not q:
        return
    table, n, every = _table(n_chains, dict(q0=q0, q=q, p=p, grad=grad, z=z, p0=p0), q)
    _hip.require_device(*(every + [state, ksum, rng_state]))
    (library or lib()).call("zs_hmc_move" + _sfx(q[0].dtype), int(kind), table, len(q), n, int(n_chains), _hip.ptr(state),
                            _hip.ptr(ksum), _binding.u64(seed), _binding.u64(call), _hip.ptr(rng_state), _hip.stream_for(q[0]))


def decide(chunks, n_chains, logp0, logp1, u, state, out, accept, adapting, delta, gamma, t0, kappa, seed=0, call=0,
           rng_state=None, library=None):
    """The accept decision of all chains and the step-size update, one launch.  ``chunks``: a list of (k0, k1, slots) -- the
    kinetic workspaces written by the BEGIN and END of every chunk; ``out``: float64[5 * n_chains]; ``accept``: int32[n_chains]."""
    table = (HmcChunk * max(len(chunks), 1))()
    every = [logp0, logp1, u, state, out, accept, rng_state]
    for e, (k0, k1, slots) in zip(table, chunks):
        e.k0, e.k1, e.slots, e.is_f64 = _hip.ptr(k0), _hip.ptr(k1), int(slots), int(k0.dtype == torch.float64)
        every += [k0, k1]
    _hip.require_device(*every)
    (library or lib()).call("zs_hmc_decide" + _sfx(logp0.dtype), table, len(chunks), int(n_chains), _hip.ptr(logp0), _hip.ptr(logp1),
                            _hip.ptr(u), _hip.ptr(state), _hip.ptr(out), _hip.ptr(accept), int(bool(adapting)), float(delta),
                            float(gamma), float(t0), float(kappa), _binding.u64(seed), _binding.u64(call), _hip.ptr(rng_state),
                            _hip.stream_for(logp0))


def select(n_chains, q0, q, q_out, accept, library=None):
    """q_out = accept[chain] ? q : q0 over the tensors of one chunk, one launch."""
    if not q:
        return
    table, n, every = _table(n_chains, dict(q0=q0, q=q, q_out=q_out), q)
    _hip.require_device(*(every + [accept]))
    (library or lib()).call("zs_hmc_select" + _sfx(q[0].dtype), table, len(q), n, int(n_chains), _hip.ptr(accept),
                            _hip.stream_for(q[0]))
