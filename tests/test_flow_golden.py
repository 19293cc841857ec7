"""The package's flow layers, FlowDistribution and ELBO(transform=) against recorded runs of the reference's
(tests/golden/flow/, made by gen_flow_golden.py on the models of tests/flow_models.py, weights stored in the fixtures).

Tolerance per quantity q, elementwise:  |got - q32| <= 16 gap_q + 2^-21 max|q32|,  gap_q = max|q32 - q64| being the reference's
own float32-versus-float64 distance on that quantity, recorded in the fixture (formed as tests/test_mcmc_golden.py forms it).
The kernels round each written operation once, like the reference's separate torch ops, but the fused tail and the scaling's
column sum add in another order and use the device's exp / log: a different realisation of the same rounding process, and
the maximum over a few dozen elements of one realisation understates another's tail; 16 covers that.  The bounds stay between
1e-7 and 4e-5 absolute: a dropped (1 - mask), a wrong sign of the shift or a missing log-det moves a value by 1e-1 or more."""
import os

import numpy as np
import pytest
import torch

import flow_models as M
from conftest import GOLDEN
from flow_host import fdev  # noqa: F401


def _load(name):
    return np.load(os.path.join(GOLDEN, "flow", "g_flow_%s.npz" % name))


def _state(g, module, dev):
    keys = list(module.state_dict().keys())
    assert sorted("w_" + k for k in keys) == sorted(f for f in g.files if f.startswith("w_")), "state_dict keys differ from the reference's"
    module.load_state_dict({k: torch.tensor(g["w_" + k]) for k in keys}, strict=True)
    return module.to(dev)


def _check(g, key, got):
    want = g[key]
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (key, got.shape, want.shape, got.dtype)
    tol = 16.0 * float(g["gap_" + key]) + 2.0 ** -21 * float(np.abs(want).max())
    err = float(np.abs(got.astype(np.float64) - want).max()) if want.size else 0.0
    print("%s: max err %.3e, tolerance %.3e" % (key, err, tol))
    assert err <= tol, (key, err, tol)


def _check_grads(g, prefix, module):
    recorded = sorted(f for f in g.files if f.startswith(prefix + "g_") and not f.startswith("gap_"))
    named = dict(module.named_parameters())
    assert recorded == sorted(prefix + "g_" + k for k, p in named.items() if p.grad is not None)
    for key in recorded:
        _check(g, key, named[key[len(prefix) + 2:]].grad)


@pytest.mark.parametrize("kind", M.LAYERS)
def test_layers_reproduce_the_reference(fdev, kind):
    import zhusuan.invertible as inv
    g = _load("layer_" + kind)
    layer = _state(g, M.make_layer(inv, kind), fdev)
    x, gy = torch.tensor(g["x"], device=fdev), torch.tensor(g["gy"], device=fdev)
    for prefix, reverse in (("fwd_", False), ("inv_", True)):
        for p in layer.parameters():
            p.grad = None
        values_only = prefix + "gx" not in g.files
        assert values_only == (kind == "made" and reverse)
        leaf = x.clone().requires_grad_(not values_only)
        if values_only:
            with torch.no_grad():
                y, ld = layer(leaf * 1.0, reverse=True)
        else:
            y, ld = layer(leaf * 1.0, reverse=reverse)
        _check(g, prefix + "y", y)
        assert (ld is None) == (prefix + "ld" not in g.files)
        if ld is not None:
            _check(g, prefix + "ld", ld)
        if values_only:
            continue
        loss = (y * gy).sum() + (M.LD_WEIGHT * ld.sum() if ld is not None else 0.0)
        loss.backward()
        _check(g, prefix + "gx", leaf.grad)
        _check_grads(g, prefix, layer)


def test_nice_log_prob_reproduces_the_reference(fdev):
    import zhusuan as zs
    import zhusuan.invertible as inv
    import zhusuan.distributions as dists
    from zhusuan.framework.bn import BayesianNet
    g = _load("nice")
    net = _state(g, M.make_nice(inv, dists, BayesianNet, device=fdev), fdev)
    x = torch.tensor(g["x"], device=fdev).requires_grad_(True)
    lp = net(x * 1.0)
    assert "zs_flow_tail" in zs.explain(net.nodes["x"].dist)
    _check(g, "lp", lp)
    (-lp.mean()).backward()
    _check(g, "gx", x.grad)
    _check_grads(g, "", net)


def test_elbo_with_a_transform_reproduces_the_reference(fdev):
    import zhusuan as zs
    import zhusuan.invertible as inv
    import zhusuan.distributions as dists
    from zhusuan.framework.bn import BayesianNet
    from zhusuan.variational.elbo import ELBO
    g = _load("elbo")
    model = _state(g, M.make_elbo(inv, dists, BayesianNet, ELBO, device=fdev), fdev)
    draws = [g["draw_%02d" % i] for i in range(int(g["n_draws"]))]
    with zs.inject_epsilon(draws):          # strict: every recorded draw is consumed, in the reference's call order
        loss = model({'x': torch.tensor(g["x"], device=fdev)})
    _check(g, "loss", loss)
    loss.backward()
    _check_grads(g, "", model)
