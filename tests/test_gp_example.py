"""examples/svgp.py, a sparse variational Gaussian process over a GPConditional node, at its smallest size on the GPU (seeded:
the same losses every run)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_example_runs_at_a_tiny_size():
    from examples import svgp
    losses, params, objective = svgp.main(steps=20, n_data=33, dim=1, inducing=17, particles=5, device="cuda:0", log_every=0)
    assert len(losses) == 20 and all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]
    for net in (objective.variational, objective.generator):
        assert net.nodes['f'].dist.last_path["path"].startswith("zs_gp_prepare") and net.nodes['f'].dist.last_path["why"] is None
    assert all(p.grad is not None and bool(torch.isfinite(p).all()) for p in params.values())
