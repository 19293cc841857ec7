"""pytest plugin used only by tests/test_flow_reference_suite.py: as tests/ref_plugin.py, `import zhusuan` resolves to THIS
package with the CPU oracle library as kernel back-end; in addition the flow kernels are the torch restatement of
tests/flow_host.py, and the torch seed is fixed (ZS_FLOW_SUITE_SEED)."""
import os

from ref_plugin import pytest_configure as _base_configure


def pytest_configure(config):
    _base_configure(config)
    import torch
    import flow_host
    torch.manual_seed(int(os.environ.get("ZS_FLOW_SUITE_SEED", "0")))
    flow_host.install()
