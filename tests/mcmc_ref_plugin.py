"""pytest plugin used only by tests/test_mcmc_reference_suite.py: as tests/ref_plugin.py, `import zhusuan` resolves to THIS
package with the CPU oracle library as kernel back-end; in addition the samplers' update function is the torch restatement
of tests/mcmc_host.py, and the torch seed and the host Philox seed are fixed (ZS_MCMC_SUITE_SEED)."""
import os

from ref_plugin import pytest_configure as _base_configure


def pytest_configure(config):
    _base_configure(config)
    import torch
    import host_backend
    import mcmc_host
    seed = int(os.environ.get("ZS_MCMC_SUITE_SEED", "0"))
    torch.manual_seed(seed)
    host_backend.manual_seed(seed)
    mcmc_host.install()
