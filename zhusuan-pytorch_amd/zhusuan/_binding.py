"""What every ctypes binding of this package shares: the loaded-library class, the lazy ``lib(path=None)`` contract of the
satellite libraries, the float32 / float64 suffix, the 64-bit mask of a Philox (seed, call) and the pointer table of a flat
index space.  ``_hip.py`` (main library), ``_mcmc_hip.py``, ``_flow_hip.py``, ``_hmc_hip.py`` and ``_cat_hip.py`` hold only what is their own:
constants, ``ctypes.Structure``s, a prototype table and their marshalling functions."""
import ctypes
import os

import torch

ERRORS = {-1: "invalid argument (ZS_EINVAL)", -2: "not supported (ZS_ENOTSUP)"}


class Library(object):
    """A loaded shared object exporting one of the zs_* C ABIs (binding the symbols needs no GPU).

    ``who``: the label of the messages; ``what`` and ``make_target`` (or ``build_hint``, the whole "run ..." advice): the words of
    the missing-file message; ``abi_symbol`` must return ``abi_version``; ``prototypes``: symbol -> ``(restype, argtypes)``, or
    ``argtypes`` alone for an entry point that returns int (0 = ok), reached through ``raw`` / ``call``; ``errors``: return
    code -> text for ``call`` (anything else is a HIP error)."""

    def __init__(self, path, *, who, abi_symbol, abi_version, prototypes, make_target=None, errors=None, what="kernel library",
                 build_hint=None):
        if not os.path.exists(path):
            hint = build_hint or ("`make -C zhusuan-pytorch_amd/csrc %s` (or `python -c 'import __graft_entry__ as g; g.build()'`)"
                                  % make_target)
            raise RuntimeError("%s (MI355X build): %s not found at %s -- run %s. There is no CPU fallback."
                               % (who, what, path, hint))
        self.path = path
        self.cdll = ctypes.CDLL(path)
        self._errors = ERRORS if errors is None else errors
        got = self.bind(abi_symbol, [])()
        if got != abi_version:
            raise RuntimeError("%s: %s has ABI version %d, expected %d" % (who, path, got, abi_version))
        self._fn = dict((name, self.bind(name, proto)) for name, proto in prototypes.items())

    def bind(self, name, proto):
        """Set the prototype of symbol ``name`` and return the function (AttributeError if the file lacks it)."""
        fn = getattr(self.cdll, name)
        fn.restype, fn.argtypes = proto if isinstance(proto, tuple) else (ctypes.c_int, proto)
        return fn

    def _error_text(self, rc):
        return self._errors.get(rc, "HIP error")

    def raw(self, name, *args):
        """The entry point's own return value (a return code: 0 = ok)."""
        return self._fn[name](*args)

    def call(self, name, *args):
        rc = self._fn[name](*args)
        if rc != 0:
            raise RuntimeError("%s failed with code %d: %s" % (name, rc, self._error_text(rc)))


def lazy_lib(module, load, path=None):
    """The ``lib(path=None)`` of a satellite binding.  ``module``: its ``globals()``, holding ``LIB_PATH`` and the cache
    ``_LIB`` (both read at call time); ``load(path)`` builds its Library.  The in-tree file is loaded once and cached; an
    explicit ``path`` loads a fresh object and leaves the cached one alone."""
    if path is not None:
        return load(path)
    if module["_LIB"] is None:
        module["_LIB"] = load(module["LIB_PATH"])
    return module["_LIB"]


def suffix(dtype, message):
    """"_f32" or "_f64": every compute entry point exists under both.  ``message``: the caller's own words, with one %s for
    any other dtype."""
    if dtype == torch.float32:
        return "_f32"
    if dtype == torch.float64:
        return "_f64"
    raise RuntimeError(message % dtype)


def both(prototypes):
    """name -> argtypes, without suffix, as name_f32 and name_f64 with the same argument list."""
    return dict((name + sfx, args) for name, args in prototypes.items() for sfx in ("_f32", "_f64"))


def u64(x):
    """A Python int as the uint64_t of a Philox seed or call id."""
    return int(x) & 0xFFFFFFFFFFFFFFFF


def flat_table(struct, columns, ref, who, n_chains=None):
    """The host table of a launch over a flat index space: one ``struct`` row per tensor of ``ref``.  ``columns`` maps a field
    name to a list of tensors like ``ref`` (entries, or the whole list, may be None: the field stays NULL); ``start`` is the
    running element count and, when ``n_chains`` is given, ``row`` the elements per chain.  Only addresses are taken.
    Returns (table, number of elements, every tensor in it)."""
    k = len(ref)
    table = (struct * max(k, 1))()
    every, start = [], 0
    for i in range(k):
        e = table[i]
        for name, col in columns.items():
            t = col[i] if col is not None else None
            if t is None:
                continue
            if t.dtype != ref[0].dtype or t.numel() != ref[i].numel() or not t.is_contiguous():
                raise RuntimeError("%s: operands of one latent must be contiguous, of one dtype and one size" % who)
            every.append(t)
            setattr(e, name, t.data_ptr())
        e.start = start
        if n_chains is not None:
            e.row = ref[i].numel() // n_chains
        start += ref[i].numel()
    return table, start, every
