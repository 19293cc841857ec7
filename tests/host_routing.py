"""TEST INFRASTRUCTURE shared by the seven tests/*_host.py modules: the plumbing that puts their torch restatements in place of
the functions of a satellite binding (which the package looks up on the binding module at call time), the record of the calls
made through a binding, the fixtures that follow the suite's ``dev``, the device check of the restatements and the call into the
C oracle's Philox streams.  The package itself contains no such routing."""
import collections
import contextlib
import importlib

import pytest
import torch

Call = collections.namedtuple("Call", "name args kwargs")


def shapes(a):
    """``a`` with every tensor replaced by its shape, through lists, tuples and dicts; everything else as it is."""
    if isinstance(a, torch.Tensor):
        return tuple(a.shape)
    if isinstance(a, (list, tuple)):
        return type(a)(shapes(v) for v in a)
    if isinstance(a, dict):
        return {k: shapes(v) for k, v in a.items()}
    return a


class _Noted(object):
    """What ``Router.recording()`` / ``count()`` put on the binding module: notes the call, then calls ``fn``."""

    def __init__(self, name, fn, note):
        self.name, self.fn, self.note = name, fn, note

    def __call__(self, *args, **kwargs):
        self.note(self.name, args, kwargs)
        return self.fn(*args, **kwargs)


class Router(object):
    """``install()`` replaces the attributes ``functions`` (name -> replacement) of module ``module_name`` and remembers the
    originals of the first install; ``uninstall()`` puts exactly those back.  Both are idempotent.  ``recording()`` and
    ``count()`` observe the calls made through those attributes, whatever they hold: the restatements on the host, the real
    functions on the GPU."""

    def __init__(self, module_name, functions):
        self.module_name = module_name
        self.functions = dict(functions)
        self._saved = None

    def _slot(self, name):
        """(holder, attribute) of the binding's function ``name``: the module, or the innermost open recording around it."""
        holder, attr = importlib.import_module(self.module_name), name
        while isinstance(getattr(holder, attr), _Noted):
            holder, attr = getattr(holder, attr), "fn"
        return holder, attr

    def install(self):
        if self._saved is None:
            self._saved = {n: getattr(*self._slot(n)) for n in self.functions}
        for n, f in self.functions.items():
            setattr(*self._slot(n), f)

    def uninstall(self):
        if self._saved is None:
            return
        for n, f in self._saved.items():
            setattr(*self._slot(n), f)
        self._saved = None

    @contextlib.contextmanager
    def _noting(self, note):
        module = importlib.import_module(self.module_name)
        mine = {n: _Noted(n, getattr(module, n), note) for n in self.functions}
        for n, w in mine.items():
            setattr(module, n, w)
        try:
            yield
        finally:
            for n, w in mine.items():
                setattr(module, n, w.fn)          # what it found; what an install() inside the block put there, if any

    @contextlib.contextmanager
    def recording(self):
        """The list of the calls made through the binding inside the block, one ``Call(name, args, kwargs)`` each, tensors as
        their shapes.  Nests, and sees the function that actually runs whether the router is installed before or inside."""
        calls = []
        with self._noting(lambda name, args, kwargs: calls.append(Call(name, shapes(args), shapes(kwargs)))):
            yield calls

    @contextlib.contextmanager
    def count(self):
        """``with router.count() as c:`` -- c[name] counts the calls of every function of the binding made inside."""
        counts = {n: 0 for n in self.functions}

        def note(name, args, kwargs):
            counts[name] += 1
        with self._noting(note):
            yield counts


def host_only(who, tensors):
    """The restatements' device check: every tensor of ``tensors`` (nested lists flattened, ``None`` skipped) is on the CPU."""
    for t in tensors:
        if isinstance(t, (list, tuple)):
            host_only(who, t)
        elif t is not None and t.device.type != "cpu":
            raise RuntimeError("tests/%s: host restatement installed but tensor is on %s" % (who, t.device))


def routed(dev, *routers):
    """Body of the ``Xdev`` fixtures (``yield from routed(dev, router, ...)``): the suite's ``dev`` (host and hip) with the
    bindings routed accordingly -- the restatements on the host, the real functions on the GPU."""
    if dev.type != "cpu":
        for r in routers:
            r.uninstall()
        yield dev
        return
    with contextlib.ExitStack() as stack:
        for r in routers:
            r.install()
            stack.callback(r.uninstall)
        yield dev


def dev_fixture(name, *routers, doc=None):
    """The pytest fixture ``name``: the suite's ``dev`` with ``routers`` routed accordingly."""
    def fixture(dev):
        yield from routed(dev, *routers)
    fixture.__doc__ = doc or "The suite's ``dev`` fixture (host and hip) with the bindings routed accordingly."
    return pytest.fixture(name=name)(fixture)


@contextlib.contextmanager
def host(*routers):
    """The host back-end for a test that does not take ``dev``: the C oracle behind the main binding, then ``routers``."""
    import conftest
    import host_backend
    host_backend.install(conftest.host_kernel_library())
    try:
        yield from routed(torch.device("cpu"), *routers)
    finally:
        host_backend.uninstall()


def philox(name, n, seed, call, rng_state=None):
    """Elements [0, n) of the oracle's Philox stream ``name`` (zs_philox_normal_f32 / zs_philox_uniform_f32; float32, CPU)."""
    import conftest
    out = torch.empty(n, dtype=torch.float32)
    conftest.host_kernel_library().call(name, out.data_ptr(), n, int(seed) & 0xFFFFFFFFFFFFFFFF, int(call) & 0xFFFFFFFFFFFFFFFF,
                                        None if rng_state is None else rng_state.data_ptr(), None)
    return out
