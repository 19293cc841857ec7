"""examples/nf_vae.py at the tiny sizes of tests/test_flow_examples.py on both back-ends: two training steps with finite losses,
the transform trained, the reference's default sizes in ``build``'s signature; and with the same seed and injected draws the
first planar loss equals that of examples/flow_vae.py, whose planar layer is the plain torch module."""
import inspect
import math

import pytest
import torch

from nf_host import ndev  # noqa: F401


@pytest.mark.parametrize("method", ["Planar", "HouseHolder"])
def test_nf_vae_trains(ndev, method):
    from examples import nf_vae
    import zhusuan as zs
    torch.manual_seed(0)
    model = nf_vae.build(method, 4, 6, 5, 8, device=ndev, n_planar=3, n_householder=2)
    assert isinstance(model.transform, zs.PlanarFlow if method == "Planar" else zs.HouseholderFlow)
    x = (torch.rand(8, 6, generator=torch.Generator().manual_seed(1)) < 0.5).float().to(ndev)
    before = [p.detach().clone() for p in model.transform.parameters()]
    losses = nf_vae.train(model, x, batch=4, steps=2)
    assert len(losses) == 2 and all(math.isfinite(v) for v in losses)
    assert all(not torch.equal(a, b) for a, b in zip(before, model.transform.parameters())), "the transform did not train"
    d = {n: p.default for n, p in inspect.signature(nf_vae.build).parameters.items()}
    assert (d["method"], d["batch_size"], d["z_dim"], d["hidden"], d["n_planar"], d["n_householder"]) == ("Planar", 64, 40, 500, 1, 5)
    with pytest.raises(NotImplementedError):
        nf_vae.build("NICE", 4, 6, 5, 8, device=ndev)


def test_the_first_planar_loss_is_flow_vaes(ndev):
    """same seed, same injected draws: examples.flow_vae's plain torch planar layer and the package's give the same loss, within
    the value bar of tests/test_flow_elbo.py (1e-6 of 1 + |loss|)"""
    import zhusuan as zs
    from examples import flow_vae, nf_vae
    g = torch.Generator().manual_seed(9)
    x = (torch.rand(4, 6, generator=g) < 0.5).float().to(ndev)
    eps = [torch.randn(4, 5, generator=g).to(ndev) for _ in range(2)]
    losses = []
    for module in (flow_vae, nf_vae):
        torch.manual_seed(0)
        model = module.build("Planar", 4, 6, 5, 8, device=ndev)
        with zs.inject_epsilon(eps):
            losses.append(model({"x": x}).detach().double().cpu())
    assert bool(torch.isfinite(losses[0])) and float((losses[0] - losses[1]).abs()) <= 1e-6 * (1.0 + float(losses[0].abs())), losses
