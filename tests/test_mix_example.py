"""examples/vamp_vae.py, a VAE whose prior is a NormalMixture over the encoder's pseudo-inputs, at a tiny size on the GPU."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_example_runs_at_a_tiny_size():
    from examples import vamp_vae
    bounds, model = vamp_vae.main(k=2, steps=3, batch=8, device="cuda:0", log_every=0, x_dim=12, z_dim=5, hidden=16, n_components=17)
    assert len(bounds) == 3 and all(math.isfinite(b) for b in bounds)
    gen = model.generator
    logits, mean, logstd = gen.prior()
    assert tuple(logits.shape) == (17,) and tuple(mean.shape) == tuple(logstd.shape) == (17, 5)
    prior = gen.nodes["z"].dist
    assert prior.last_path["path"].startswith("zs_mix_prepare") and prior.last_workspaces["grad_x_ran"]
    assert prior.last_workspaces["grad_params_workspace_elems"] > 0
    assert gen.pseudo_inputs.grad is not None and bool(torch.isfinite(gen.pseudo_inputs.grad).all())
    assert all(bool(torch.isfinite(p).all()) for p in model.parameters())
