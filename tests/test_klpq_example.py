"""examples/rws_sbn.py at a tiny size on both back-ends: wake-wake training over 30 steps at the example's default seed raises
the importance-sampled log-likelihood on average (first-10 mean < last-10 mean; the host back-end's two values are recorded in
tests/README_klpq.md), and the one-hot latent, the vimco switch and the sleep phase run and give finite gradients that reach both
nets."""
import inspect

import pytest
import torch

import cat_host
import host_backend
import host_routing
import klpq_host
import zhusuan as zs

TINY = dict(x_dim=16, h1=8, h2=4, n_latents=2, n_categories=4, n_samples=5)


# ``kdev`` with the categorical binding routed as well (the example's one-hot latent)
edev = host_routing.dev_fixture("edev", klpq_host.router, cat_host.router)


def run(dev, steps, **kw):
    from examples import rws_sbn as E
    seed = inspect.signature(E.main).parameters['seed'].default
    host_backend.manual_seed(seed)
    return E.main(steps=steps, batch=8, device=dev, log_every=0, **kw, **TINY)


def test_wake_wake_raises_the_importance_sampled_log_likelihood(edev):
    h = run(edev, 30, estimator='rws', latent='bernoulli')
    first, last = sum(h[:10]) / 10, sum(h[-10:]) / 10
    print("is_loglikelihood: first 10 steps %.4f, last 10 steps %.4f" % (first, last))
    assert len(h) == 30 and all(v == v and abs(v) < 1e6 for v in h)
    assert last > first


@pytest.mark.parametrize("estimator,latent,sleep", [('rws', 'onehot', False), ('rws', 'bernoulli', True), ('vimco', 'bernoulli', False)])
def test_the_other_ways_run_and_their_gradients_reach_both_nets(edev, estimator, latent, sleep):
    from examples import rws_sbn as E
    h = run(edev, 4, estimator=estimator, latent=latent, sleep=sleep)
    assert len(h) == 4 and all(v == v and abs(v) < 1e6 for v in h)
    model = E.build(estimator, latent, batch=8, device=edev, **TINY)
    x = E.synthetic_data(8, TINY['x_dim']).to(edev)
    loss = model({'x': x})
    if sleep:
        loss = loss + model.sleep_cost(['x'], n_samples=TINY['n_samples'])
    loss.backward()
    print("explain: %s" % zs.explain(model))
    named = dict(model.named_parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in named.values())
    for net in ('generator.', 'variational.'):
        assert any(float(p.grad.abs().sum()) > 0 for n, p in named.items() if n.startswith(net)), net
