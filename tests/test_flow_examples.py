"""examples/nice.py and examples/flow_vae.py at tiny sizes on both back-ends: two training steps with a finite loss, samples of
the right shape, the reference's default sizes in ``build``'s signature."""
import inspect
import math

import pytest
import torch

from flow_host import fdev  # noqa: F401


def test_nice_trains_and_samples(fdev):
    from examples import nice
    torch.manual_seed(0)
    model = nice.build(num_coupling=3, in_out_dim=7, mid_dim=5, hidden=2, device=fdev)
    x = torch.rand(8, 7, generator=torch.Generator().manual_seed(1)).to(fdev)
    losses = nice.train(model, x, batch=4, steps=2)
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses)
    with torch.no_grad():
        s = model.sample(3)
    assert s.shape == (3, 7) and bool(torch.isfinite(s).all())
    d = {n: p.default for n, p in inspect.signature(nice.build).parameters.items()}
    assert (d["num_coupling"], d["in_out_dim"], d["mid_dim"], d["hidden"]) == (4, 784, 1000, 5)          # nice_mnist.py:45-50


@pytest.mark.parametrize("method", ["NICE", "Planar", "HouseHolder"])
def test_flow_vae_trains(fdev, method):
    from examples import flow_vae
    torch.manual_seed(0)
    model = flow_vae.build(method, 4, 6, 5, 8, device=fdev, mid_dim_flow=6, num_coupling=3, num_hidden_per_coupling=2,
                           n_householder=2)
    x = (torch.rand(8, 6, generator=torch.Generator().manual_seed(1)) < 0.5).float().to(fdev)
    before = [p.detach().clone() for p in model.transform.parameters()]
    losses = flow_vae.train(model, x, batch=4, steps=2)
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses)
    assert any(not torch.equal(a, b) for a, b in zip(before, model.transform.parameters())), "the transform did not train"
    d = {n: p.default for n, p in inspect.signature(flow_vae.build).parameters.items()}
    assert (d["batch_size"], d["z_dim"], d["mid_dim_flow"], d["num_coupling"], d["num_hidden_per_coupling"]) == (64, 40, 64, 10, 4)
    with pytest.raises(NotImplementedError):
        flow_vae.build("other", 4, 6, 5, 8, device=fdev)
