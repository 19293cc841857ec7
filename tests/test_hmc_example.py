"""examples/gaussian_hmc.py, the counterpart of the reference's toy Gaussian example run with HMC, on both back-ends."""
import math

import torch

import hmc_host
import host_backend
import host_routing
from hmc_host import hdev  # noqa: F401


def test_example_runs_at_a_tiny_size(hdev):
    from examples import gaussian_hmc
    host_backend.manual_seed(0)
    r = gaussian_hmc.run(n_x=3, n_chains=4, n_iters=6, n_leapfrogs=2, device=hdev)
    assert tuple(r["samples"].shape) == (3, 4, 3) and r["samples"].device == hdev and bool(torch.isfinite(r["samples"]).all())
    assert tuple(r["mean"].shape) == (3,) and tuple(r["std"].shape) == (3,) and bool(torch.isfinite(r["std"]).all())
    assert torch.allclose(r["expected_std"], torch.tensor([1.0, 0.5, 1.0 / 3], dtype=torch.float64))
    assert 0.0 <= r["acceptance"] <= 1.0 and math.isfinite(r["step_size"]) and r["step_size"] > 0


def test_example_runs_with_the_reference_examples_default_sizes_on_the_host():
    """n_x = 1, one chain, 200 iterations, 20 leapfrog steps: the reference example's parameter block."""
    from examples import gaussian_hmc
    with host_routing.host(hmc_host.router):
        host_backend.manual_seed(1)
        r = gaussian_hmc.run(device="cpu")
    assert tuple(r["samples"].shape) == (100, 1, 1) and bool(torch.isfinite(r["samples"]).all())
    # 100 correlated draws of one chain: a loose sanity band around the unit standard deviation, not a test of the sampler
    assert 0.3 < float(r["std"]) < 3.0 and abs(float(r["mean"])) < 1.5 and r["acceptance"] > 0.3
