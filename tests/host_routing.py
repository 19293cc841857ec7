"""TEST INFRASTRUCTURE shared by tests/mcmc_host.py, tests/hmc_host.py and tests/flow_host.py: the plumbing that puts their
torch restatements in place of the functions of a satellite binding (which the package looks up on the binding module at call
time), the fixture body that follows the suite's ``dev``, and the call into the C oracle's Philox streams.  The package itself
contains no such routing."""
import importlib

import torch


class Router(object):
    """``install()`` replaces the attributes ``functions`` (name -> replacement) of module ``module_name`` and remembers the
    originals of the first install; ``uninstall()`` puts exactly those back.  Both are idempotent."""

    def __init__(self, module_name, functions):
        self.module_name = module_name
        self.functions = dict(functions)
        self._saved = None

    def install(self):
        module = importlib.import_module(self.module_name)
        if self._saved is None:
            self._saved = {n: getattr(module, n) for n in self.functions}
        for n, f in self.functions.items():
            setattr(module, n, f)

    def uninstall(self):
        if self._saved is None:
            return
        module = importlib.import_module(self.module_name)
        for n, f in self._saved.items():
            setattr(module, n, f)
        self._saved = None


def routed(router, dev):
    """Body of the ``mdev`` / ``hdev`` / ``fdev`` fixtures (``yield from routed(router, dev)``): the suite's ``dev`` (host and
    hip) with the binding routed accordingly -- the restatement on the host, the real functions on the GPU."""
    if dev.type == "cpu":
        router.install()
        try:
            yield dev
        finally:
            router.uninstall()
    else:
        router.uninstall()
        yield dev


def philox(name, n, seed, call, rng_state=None):
    """Elements [0, n) of the oracle's Philox stream ``name`` (zs_philox_normal_f32 / zs_philox_uniform_f32; float32, CPU)."""
    import conftest
    out = torch.empty(n, dtype=torch.float32)
    conftest.host_kernel_library().call(name, out.data_ptr(), n, int(seed) & 0xFFFFFFFFFFFFFFFF, int(call) & 0xFFFFFFFFFFFFFFFF,
                                        None if rng_state is None else rng_state.data_ptr(), None)
    return out
