"""examples/fullcov_vae.py at a tiny size on both back-ends: the ELBO over 30 steps at the example's default seed increases on
average (first-10 mean < last-10 mean; the host back-end's two values are recorded in tests/README_mvn.md), and the
importance-weighted variant runs and gives finite gradients that reach the encoder's L head."""
import inspect

import torch

import host_backend
import zhusuan as zs
from mvn_host import vdev  # noqa: F401

TINY = dict(x_dim=16, z_dim=4, hidden=16)


def run(k, dev, steps):
    from examples import fullcov_vae as E
    seed = inspect.signature(E.main).parameters['seed'].default
    host_backend.manual_seed(seed)
    return E.main(k, steps=steps, batch=8, device=dev, log_every=0, **TINY)


def test_the_elbo_increases_on_average(vdev):
    b = run(1, vdev, 30)
    first, last = sum(b[:10]) / 10, sum(b[-10:]) / 10
    print("ELBO: first 10 steps %.4f, last 10 steps %.4f" % (first, last))
    assert all(v == v and abs(v) < 1e6 for v in b)
    assert last > first


def test_the_importance_weighted_variant_trains(vdev):
    from examples import fullcov_vae as E
    b = run(5, vdev, 6)
    assert len(b) == 6 and all(v == v and abs(v) < 1e6 for v in b)
    model = E.build(5, device=vdev, **TINY)
    x = E.synthetic_data(8, TINY['x_dim']).to(vdev)
    loss = model({'x': x})
    loss.backward()
    print("explain: %s" % zs.explain(model))
    named = dict(model.named_parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in named.values())
    heads = [n for n in named if 'tril_head' in n]
    assert heads and all(float(named[n].grad.abs().sum()) > 0 for n in heads)
