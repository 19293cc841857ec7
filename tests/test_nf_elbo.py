"""``ELBO(transform=PlanarFlow(5, 3, name='z'), transform_var=['z'])`` and the Householder variant with
``auxillary_var=['z_logits']`` on both back-ends, at B = 4, x = 6, z = 5.

Truth: the same nets evaluated node by node in the reference's order under the same injected draws, as in
tests/test_flow_elbo.py and to its bars: values to 1e-6 and gradients to 1e-5 of 1 + the tensor's largest magnitude."""
import pytest
import torch

import nf_host
from nf_host import ndev  # noqa: F401
from test_flow_elbo import B, X, Z, H, data, node_by_node, close


def build(method, dev, estimator="sgvb", seed=0):
    import zhusuan as zs
    from zhusuan.variational.elbo import ELBO
    from examples import flow_vae, vae_mnist
    torch.manual_seed(seed)
    generator, variational = vae_mnist.Generator(X, Z, B, H), flow_vae.Variational(X, Z, B, H)
    if method == "Planar":
        return ELBO(generator, variational, estimator=estimator, transform=zs.transform.PlanarFlow(Z, 3, name='z'),
                    transform_var=['z']).to(dev)
    return ELBO(generator, variational, estimator=estimator, transform=zs.transform.HouseholderFlow(Z, H, 2, name='z'),
                transform_var=['z'], auxillary_var=['z_logits']).to(dev)


@pytest.mark.parametrize("method", ["Planar", "HouseHolder"])
def test_value_and_gradients_equal_the_node_by_node_evaluation(ndev, method):
    import zhusuan as zs
    model = build(method, ndev)
    x, eps = data(ndev)
    with zs.inject_epsilon(eps):
        loss = model({"x": x})
    assert loss.shape == () and bool(torch.isfinite(loss))
    assert "a transform is set" in zs.explain(model)
    assert ("P1 zs_nf_planar_fwd" if method == "Planar" else "H1 zs_nf_householder_fwd") in zs.explain(model.transform)
    params = list(model.parameters())
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    loss2, log_det = node_by_node(model, x, eps)
    grads2 = torch.autograd.grad(loss2, params, allow_unused=True)
    close(loss, loss2, 1e-6, "loss")
    assert log_det.shape == ((B, 1) if method == "Planar" else (1, 1))
    if method == "Planar":
        assert float(log_det.detach().abs().sum()) > 0.0
    for (n, _), a, b in zip(model.named_parameters(), grads, grads2):
        assert (a is None) == (b is None), n
        if a is not None:
            close(a, b, 1e-5, n)
    # every parameter of the transform is reached
    tnames = [n for n, _ in model.named_parameters() if n.startswith("transform.")]
    assert len(tnames) == (3 if method == "Planar" else 4)
    assert all(g is not None and float(g.abs().sum()) > 0 for (n, _), g in zip(model.named_parameters(), grads) if n in tnames)
    # the generator saw the TRANSFORMED latent
    assert not torch.equal(model.generator.observed["z"], model.variational.nodes["z"].dist.sample_cache)


def test_the_elbo_equals_the_plain_torch_transform(ndev):
    """the package's planar stack inside ELBO against the example's PF layers applied in a loop with the log-dets summed"""
    import zhusuan as zs
    from test_nf_layers import example_planar
    model = build("Planar", ndev)
    x, eps = data(ndev)
    with zs.inject_epsilon(eps):
        loss = model({"x": x})
    flow = model.transform

    class Plain(torch.nn.Module):
        def forward(self, z, **kw):
            out, ld = example_planar(z[0], flow.u, flow.w, flow.b)
            return {"z": out}, ld
    model.transform = Plain()
    with zs.inject_epsilon(eps):
        loss2 = model({"x": x})
    close(loss, loss2, 1e-5, "loss")


def test_reinforce_costs_no_finish_for_the_log_det_and_is_finite(ndev):
    """'reinforce' drops the log-det: its cotangent reaches P1b as NULL, and a doubled log-det returns the same cost"""
    import zhusuan as zs
    x, eps = data(ndev)
    model = build("Planar", ndev, "reinforce")
    with nf_host.recording() as calls:
        with zs.inject_epsilon(eps):
            la = model({"x": x}, variance_reduction=False)
        la.backward()
    assert bool(torch.isfinite(la))
    bwd = [c for c in calls if c[0] == "planar_bwd"]
    assert [c[0] for c in calls].count("planar_fwd") == 1 and len(bwd) <= 1
    assert all(c[2]["gld"] is None for c in bwd)          # the log-det did not enter the cost
    inner = model.transform

    class Doubled(torch.nn.Module):
        def forward(self, z, **kw):
            out, ld = inner(z, **kw)
            return out, 2.0 * ld + 5.0
    model.transform = Doubled()
    with zs.inject_epsilon(eps):
        lb = model({"x": x}, variance_reduction=False)
    assert torch.equal(la, lb)
