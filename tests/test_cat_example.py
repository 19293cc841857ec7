"""examples/categorical_vae.py at a tiny size on both back-ends: the three ways train through the objectives as they stand, and
the VIMCO bound over 30 steps at the example's default seed does not decrease on average (first-10 mean < last-10 mean; on the
host back-end, whose Philox stream is the device's bit for bit: -10.963 -> -10.682)."""
import inspect

import pytest
import torch

import host_backend
from cat_host import cdev  # noqa: F401

TINY = dict(x_dim=16, n_latents=2, n_categories=4, hidden=16, n_samples=5)


def run(mode, dev, steps):
    from examples import categorical_vae as E
    seed = inspect.signature(E.main).parameters['seed'].default
    host_backend.manual_seed(seed)
    return E.main(mode, steps=steps, batch=8, device=dev, log_every=0, **TINY)


def test_vimco_bound_does_not_decrease_on_average(cdev):
    b = run('vimco', cdev, 30)
    first, last = sum(b[:10]) / 10, sum(b[-10:]) / 10
    print("VIMCO bound: first 10 steps %.4f, last 10 steps %.4f" % (first, last))
    assert all(v == v and abs(v) < 1e6 for v in b)
    assert first < last


@pytest.mark.parametrize("mode", ["reinforce", "sgvb"])
def test_the_other_two_ways_train(cdev, mode):
    from examples import categorical_vae as E
    b = run(mode, cdev, 6)
    assert len(b) == 6 and all(v == v and abs(v) < 1e6 for v in b)
    model = E.build(mode, device=cdev, **TINY)
    x = E.synthetic_data(8, TINY['x_dim']).to(cdev)
    loss = model({'x': x})
    loss.backward()
    grads = [p.grad for p in model.parameters()]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(float(g.abs().sum()) > 0 for n, g in zip([n for n, _ in model.named_parameters()], grads) if n.startswith('variational'))
