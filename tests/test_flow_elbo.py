"""``ELBO(transform=, transform_var=, auxillary_var=)`` on both back-ends, at B = 4, x = 6, z = 5: a three-coupling NICE flow plus a
Scaling, a planar flow and a Householder flow that reads the auxiliary variable ``z_logits`` (examples/flow_vae.py).

Truth: the same nets evaluated node by node in the reference's order (elbo.py:86-132 of thuwzy/ZhuSuan-PyTorch) under the same
injected draws.  Both sides run the same kernels on the same numbers; they differ in nothing but the order in which autograd
accumulates gradients, so values are held to 1e-6 and gradients to 1e-5 of the tensor's largest magnitude (a handful of
float32 roundings)."""
import pytest
import torch

import flow_host
import truth
from flow_host import fdev  # noqa: F401

B, X, Z, H = 4, 6, 5, 8


def build(method, dev, estimator="sgvb", seed=0):
    from examples import flow_vae
    torch.manual_seed(seed)
    model = flow_vae.build(method, B, X, Z, H, device=dev, mid_dim_flow=6, num_coupling=3, num_hidden_per_coupling=2,
                           n_householder=2)
    if estimator != "sgvb":
        from zhusuan.variational.elbo import ELBO
        model = ELBO(model.generator, model.variational, estimator=estimator, transform=model.transform,
                     transform_var=model.transform_var, auxillary_var=model.auxillary_var).to(dev)
    if method == "NICE":
        with torch.no_grad():
            model.transform.flow.layers[-1].log_scale.normal_()
    return model


def data(dev):
    g = truth.gen(9)
    x = (torch.rand(B, X, generator=g) < 0.5).float().to(dev)
    eps = [torch.randn(B, Z, generator=g).to(dev) for _ in range(2)]
    return x, eps


def node_by_node(model, x, eps, with_log_det=True):
    """elbo.py:86-132, spelled out."""
    import zhusuan as zs
    with zs.inject_epsilon(eps):
        model.variational({"x": x})
        nodes_q = model.variational.nodes
        flow_inputs = tuple([nodes_q[k].tensor for k in model.transform_var] + [model.variational.cache[k] for k in model.auxillary_var])
    output, log_det = model.transform(flow_inputs)
    observed = {k: output[k] for k in model.transform_var}
    observed["x"] = x
    model.generator(observed)
    logp, logq = model.log_joint(model.generator.nodes), model.log_joint(nodes_q)
    elbo = torch.mean(logp - logq) if logq.dim() > 0 else logp - logq
    if with_log_det:
        elbo = elbo + torch.mean(torch.sum(log_det)).squeeze()
    return -elbo, log_det


def close(a, b, tol, what=""):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * (1.0 + float(b.abs().max())), (what, float((a - b).abs().max()))


@pytest.mark.parametrize("method", ["NICE", "Planar", "HouseHolder"])
def test_value_and_gradients_equal_the_node_by_node_evaluation(fdev, method):
    import zhusuan as zs
    model = build(method, fdev)
    x, eps = data(fdev)
    assert model.transform is not None and model.transform_var == ["z"]
    assert model.auxillary_var == (["z_logits"] if method == "HouseHolder" else [])
    with zs.inject_epsilon(eps):
        loss = model({"x": x})
    assert loss.shape == () and bool(torch.isfinite(loss))
    assert "LJ1" in zs.explain(model) and "a transform is set" in zs.explain(model) and model.last_path["why"]
    params = list(model.parameters())
    grads = torch.autograd.grad(loss, params, allow_unused=True)
    loss2, log_det = node_by_node(model, x, eps)
    grads2 = torch.autograd.grad(loss2, params, allow_unused=True)
    close(loss, loss2, 1e-6, "loss")
    if method != "HouseHolder":          # (a reflection preserves volume: its log-det is a constant zero)
        assert float(log_det.detach().abs().sum()) > 0.0
    for (n, _), a, b in zip(model.named_parameters(), grads, grads2):
        assert (a is None) == (b is None), n
        if a is not None:
            close(a, b, 1e-5, n)
    # every parameter of the transform is reached
    tnames = [n for n, _ in model.named_parameters() if n.startswith("transform.")]
    assert tnames and all(g is not None for (n, _), g in zip(model.named_parameters(), grads) if n in tnames)
    # the generator saw the TRANSFORMED latent, the variational log-joint the untransformed draw
    z_q = model.variational.nodes["z"].dist.sample_cache
    assert not torch.equal(model.generator.observed["z"], z_q)


def test_reinforce_drops_the_log_det(fdev):
    import zhusuan as zs
    x, eps = data(fdev)
    a, b = build("NICE", fdev, "reinforce"), build("NICE", fdev, "reinforce")
    with torch.no_grad():
        b.transform.flow.layers[-1].log_scale.copy_(a.transform.flow.layers[-1].log_scale)
    # (these nodes reduce to scalars, for which the reference's moving-mean buffers do not broadcast: elbo.py:221)
    with zs.inject_epsilon(eps):
        la = a({"x": x}, variance_reduction=False)
    # the same model with the scaling's log-det doubled by hand in a wrapper: reinforce returns the same cost
    inner = b.transform

    class Doubled(torch.nn.Module):
        def forward(self, z, **kw):
            out, ld = inner(z, **kw)
            return out, 2.0 * ld + 5.0
    b.transform = Doubled()
    with zs.inject_epsilon(eps):
        lb = b({"x": x}, variance_reduction=False)
    assert torch.equal(la, lb) and bool(torch.isfinite(la))
    # ... while sgvb does not
    s1 = build("NICE", fdev)
    with zs.inject_epsilon(eps):
        l1 = s1({"x": x})
    inner1 = s1.transform

    class Doubled1(torch.nn.Module):
        def forward(self, z, **kw):
            out, ld = inner1(z, **kw)
            return out, 2.0 * ld + 5.0
    ld0 = float(inner1.flow.layers[-1].log_scale.detach().sum())
    s1.transform = Doubled1()
    with zs.inject_epsilon(eps):
        l2 = s1({"x": x})
    close(l2, l1 - (ld0 + 5.0), 1e-5, "sgvb adds mean(sum(log_det))")


def test_the_three_asserts(fdev):
    from zhusuan.variational.elbo import ELBO
    x, eps = data(fdev)
    model = build("NICE", fdev)
    gen, var, flow = model.generator, model.variational, model.transform
    with pytest.raises(AssertionError):          # a transformed name is observed
        model({"x": x, "z": torch.zeros(B, Z, device=fdev)})
    with pytest.raises(AssertionError):          # ... is not a node of q
        ELBO(gen, var, transform=flow, transform_var=["w"]).to(fdev)({"x": x})

    class TwoOutputs(torch.nn.Module):
        def forward(self, z, **kw):
            out, ld = flow(z, **kw)
            out["extra"] = out["z"]
            return out, ld
    with pytest.raises(AssertionError):          # the output's length differs from len(transform_var)
        ELBO(gen, var, transform=TwoOutputs(), transform_var=["z"]).to(fdev)({"x": x})


def test_without_a_transform_nothing_changes(fdev):
    import zhusuan as zs
    from zhusuan import _ops
    from zhusuan.variational.elbo import ELBO
    model = build("NICE", fdev)
    plain = ELBO(model.generator, model.variational).to(fdev)
    plain_none = ELBO(model.generator, model.variational, transform=None, transform_var=["z"]).to(fdev)
    x, eps = data(fdev)
    for m in (plain, plain_none):
        assert m.transform is None
        calls = []
        orig = _ops.LogJointScalar.apply

        def spy(spec, *tensors):
            calls.append(1)
            return orig(spec, *tensors)
        _ops.LogJointScalar.apply = spy
        try:
            with flow_host.count_launches() as c, zs.inject_epsilon(eps):
                loss = m({"x": x})
        finally:
            _ops.LogJointScalar.apply = orig
        assert calls == [1] and sum(c.values()) == 0
        assert zs.explain(m).startswith("LJ1") and m.last_path["why"] is None
    with zs.inject_epsilon(eps):
        assert torch.equal(plain({"x": x}), loss)
