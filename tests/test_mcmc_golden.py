"""The package's samplers against recorded runs of the reference's (tests/golden/mcmc/, made by gen_mcmc_golden.py): a small
BNN, SGLD / PSGLD with two latents, SGHMC first and second order with one latent and a velocity resample inside the run.

Tolerance per step t, elementwise:  |q - q32_t| <= 16 gap[t] + 2^-21 max|q32_t|,  gap[t] = max|q32_t - q64_t| being the
reference's own float32-versus-float64 distance on the same draws, recorded in the fixture.  The fused update contracts to
FMA, uses 1-ulp hardware sqrt and rcp and takes its gradient from kernels with another reduction order: a different
realisation of the same rounding process, and the maximum over ~100 elements of one realisation understates another's tail;
16 covers that.  The bound stays near 5e-6 absolute: a dropped 1/2, a wrong noise scale (sqrt(lr) = 0.03) or a stale velocity
moves q by 1e-3 or more.  (Largest distance reached: 1.2e-7 on the host back-end, 1.8e-7 on the MI355X.)"""
import os

import numpy as np
import pytest
import torch

import mcmc_models as M
from conftest import GOLDEN
from mcmc_host import mdev  # noqa: F401


def _load(case):
    g = np.load(os.path.join(GOLDEN, "mcmc", "g_mcmc_%s.npz" % case))
    return g, [g["draw_%02d" % i] for i in range(int(g["n_draws"]))]


def _check(g, t, out, worst):
    names = [str(k) for k in g["names"]]
    assert list(out.keys()) == names
    for k in names:
        want = g["q_%d_%s" % (t, k)]
        got = out[k].detach().cpu().numpy()
        assert got.shape == want.shape and got.dtype == want.dtype
        tol = 16.0 * float(g["gap"][t]) + 2.0 ** -21 * float(np.abs(want).max())
        err = float(np.abs(got.astype(np.float64) - want).max())
        worst.append((t, k, err, tol))
        print("step %d %s: max err %.3e, tolerance %.3e" % (t, k, err, tol))
        assert err <= tol, (t, k, err, tol)


def _run(dev, case, g):
    import zhusuan.mcmc
    from zhusuan.framework.bn import BayesianNet
    cls, kw, layers = M.CASES[case]
    net = M.make_net(BayesianNet, layers, device=dev)
    sampler = getattr(zhusuan.mcmc, cls)(M.LR, **kw)
    obs = {'x': torch.tensor(g["x"], device=dev), 'y': torch.tensor(g["y"], device=dev)}
    worst = []
    _check(g, 0, sampler.sample(net, obs, resample=True), worst)
    assert sampler.t == 1
    for t in range(1, M.N_UPDATES + 1):
        _check(g, t, sampler.sample(net, obs), worst)
    assert sampler.t == 1 + M.N_UPDATES


@pytest.mark.parametrize("case", list(M.CASES))
def test_injected_draws_reproduce_the_reference_step_by_step(mdev, case):
    import zhusuan
    g, draws = _load(case)
    with zhusuan.inject_epsilon(draws):         # strict: every recorded draw is consumed, in the reference's call order
        _run(mdev, case, g)


@pytest.mark.parametrize("case", list(M.CASES))
def test_reference_rng_reproduces_the_reference_from_its_seed(mdev, case):
    import zhusuan
    g, _ = _load(case)
    torch.manual_seed(int(g["seed"]))
    with zhusuan.reference_rng():
        _run(mdev, case, g)
