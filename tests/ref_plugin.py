"""pytest plugin used only by tests/reference_runs.py: makes `import zhusuan` resolve to THIS package and routes its kernel
calls to the CPU oracle library, so the reference's own unittest files can run against it on a GPU-less machine.  ZS_REF_SUITE
names the suite: "flow" adds the torch restatement of tests/flow_host.py and fixes the torch seed (ZS_FLOW_SUITE_SEED); "mcmc"
adds that of tests/mcmc_host.py and fixes the torch seed and the host Philox seed (ZS_MCMC_SUITE_SEED)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "zhusuan-pytorch_amd")):
    if p in sys.path:
        sys.path.remove(p)
    sys.path.insert(0, p)


def pytest_configure(config):
    import zhusuan
    assert zhusuan.__file__.startswith(os.path.join(ROOT, "zhusuan-pytorch_amd")), zhusuan.__file__
    from zhusuan import _hip
    import conftest
    import host_backend
    host_backend.install(conftest.host_kernel_library())
    suite = os.environ.get("ZS_REF_SUITE", "")
    if suite:
        import importlib
        import torch
        seed = int(os.environ.get("ZS_%s_SUITE_SEED" % suite.upper(), "0"))
        torch.manual_seed(seed)
        if suite == "mcmc":
            host_backend.manual_seed(seed)
        importlib.import_module(suite + "_host").install()
