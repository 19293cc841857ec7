"""MultivariateNormalLowRank and ``BayesianNet.multivariate_normal_low_rank`` (zhusuan/distributions/lowrank.py): the public
interface over the kernels of include/zs_lowrank.h.  The truth is that of tests/test_lowrank_kernel.py; the objectives are held
to the suite's rule (16 x the float32 model's own distance from float64)."""
import pytest
import torch
import torch.distributions as td

import zhusuan as zs
from zhusuan.distributions import MultivariateNormalLowRank as LowRank
from zhusuan.distributions._lowrank_functions import torch_log_prob
from zhusuan.framework.bn import BayesianNet
from zhusuan.variational.elbo import ELBO

from test_lowrank_kernel import DENSITY, case_inputs, density, mvn_log_prob
from truth import gen, held_to_the_rule

F32, F64 = torch.float32, torch.float64
WORST = {}


class Net(BayesianNet):
    def __init__(self, build):
        super().__init__()
        self.build = build

    def forward(self, observed):
        self.observe(observed)
        self.build(self)
        return self


# ------------------------------------------------------------------------------------------------ no GPU
@pytest.mark.parametrize("D,r,K,R", [(37, 5, 4, 1), (130, 17, 3, 2)])
def test_cpu_tensors_run_the_torch_composition(D, r, K, R):
    """The Woodbury composition in float64 against the dense definition: the two differ by float64 rounding only (1e-9 relative
    is some 1e5 roundings of either)."""
    assert 'MultivariateNormalLowRank' in zs.distributions.__all__ and LowRank._event_ndims == 1
    mean, W, d, x, g = case_inputs(D, r, K, R)[:5]
    t, c = density(mvn_log_prob, mean, W, d, x, g, F64), density(torch_log_prob, mean, W, d, x, g, F64)
    for n in DENSITY:
        assert float((c[n] - t[n]).abs().max()) <= 1e-9 * float(t[n].abs().max()), n
    dist = LowRank(mean, W, d)
    assert tuple(dist.batch_shape) == (R,) and (dist.n_dims, dist.rank) == (D, r)
    assert torch.equal(dist.log_prob(x), torch_log_prob(mean, W, d, x))
    assert dist.last_path["path"].startswith("torch composition") and "CPU" in zs.explain(dist)
    z = dist.sample(6)
    assert tuple(z.shape) == (6, R, D) and "CPU" in zs.explain(dist)
    with pytest.raises(ValueError):
        LowRank(mean, W[:, :-1], d)


# ------------------------------------------------------------------------------------------------ GPU
OD, OR_, OK_, OX = 70, 5, 6, 9          # the weights of one linear layer as a flat vector: two panels of the factor


def objective_setup(dev, dtype):
    g = gen(410)
    P = dict(m=0.3 * torch.randn(OD, generator=g, dtype=F64), w=torch.randn(OD, OR_, generator=g, dtype=F64) / OR_ ** 0.5,
             s=torch.randn(OD, generator=g, dtype=F64))
    P = {k: v.to(dtype).to(dev).requires_grad_(True) for k, v in P.items()}
    x, y = torch.randn(OX, OD, generator=g, dtype=F64) / OD ** 0.5, torch.randn(OX, generator=g, dtype=F64)
    return P, x.to(dtype).to(dev), y.to(dtype).to(dev)


def zs_objective(estimator, dev, eps):
    P, x, y = objective_setup(dev, F32)

    def q(net):
        net.multivariate_normal_low_rank('w', P['m'], 0.2 * P['w'], torch.exp(0.3 * P['s']), n_samples=OK_,
                                         is_reparameterized=estimator == "sgvb")

    def p(net):
        w = net.normal('w', mean=torch.zeros(OD, device=dev), std=torch.ones(OD, device=dev), n_samples=OK_, group_ndims=1)
        net.normal('y', mean=w @ x.T, std=torch.ones(OX, device=dev), group_ndims=1)
    obj = ELBO(Net(p).to(dev), Net(q).to(dev), estimator=estimator).to(dev)
    with zs.inject_epsilon([eps, eps]):          # the objectives draw every latent twice and use the second draw
        loss = obj({'y': y})
    return loss, torch.autograd.grad(loss, list(P.values())), obj.variational.nodes['w'].dist


def torch_objective(estimator, dev, dtype, eps):
    """The same model with torch.distributions on the CPU in `dtype`; the objective's own epilogue on (log p, log q)."""
    P, x, y = objective_setup("cpu", dtype)
    W, d, e = 0.2 * P['w'], torch.exp(0.3 * P['s']), eps.to(dtype)
    w = P['m'] + torch.sqrt(d) * e[:, :OD] + e[:, OD:] @ W.T
    w = w if estimator == "sgvb" else w.detach()
    logq = td.LowRankMultivariateNormal(P['m'], W, d).log_prob(w)
    logp = td.Normal(0.0, 1.0).log_prob(w).sum(-1) + td.Normal(w @ x.T, 1.0).log_prob(y).sum(-1)
    loss = getattr(ELBO(Net(None), Net(None), estimator=estimator).to(dev), estimator)(logp.to(dev), logq.to(dev))
    return loss, torch.autograd.grad(loss, list(P.values()))


@pytest.mark.gpu
@pytest.mark.parametrize("estimator", ["sgvb", "reinforce"])
def test_objectives_over_a_low_rank_latent(estimator):
    """Value and parameter gradients against the same model written with torch.distributions in float64 with the same injected
    eps, within 16 x that model's own float32-vs-float64 distance; the multiples seen are in tests/README_lowrank.md."""
    dev = torch.device("cuda:0")
    eps = torch.randn(OK_, OD + OR_, generator=gen(411))
    loss, grads, dist = zs_objective(estimator, dev, eps)
    assert "zs_lowrank_logprob" in zs.explain(dist) and dist.last_path["why"] is None
    l64, g64 = torch_objective(estimator, dev, F64, eps)
    l32, g32 = torch_objective(estimator, dev, F32, eps)
    held_to_the_rule(estimator, [("loss", loss, l32, l64)] + list(zip("mws", grads, g32, g64)), WORST)
    print("largest multiples: %s" % sorted(WORST.items()))


@pytest.mark.gpu
def test_routing_named_in_explain():
    dev = torch.device("cuda:0")
    mean, W, d, x = (t.to(F32).to(dev) for t in case_inputs(17, 5, 3, 2)[:4])
    dist = LowRank(mean, W, d)
    z = dist.sample(3)
    assert tuple(z.shape) == (3, 2, 17) and "zs_lowrank_sample" in zs.explain(dist)
    lp = dist.log_prob(x)
    want = mvn_log_prob(*(t.cpu().double() for t in (mean, W, d, x)))
    assert "zs_lowrank_logprob" in zs.explain(dist) and float((lp.cpu().double() - want).abs().max()) <= 1e-4 * float(want.abs().max())
    wide = LowRank(mean, torch.cat([W] * 13, -1), d)          # rank 65
    assert tuple(wide.sample(2).shape) == (2, 2, 17) and "zs_lowrank_max_rank" in zs.explain(wide)
    assert tuple(wide.log_prob(x).shape) == (3, 2) and wide.last_path["path"].startswith("torch composition") and "64" in zs.explain(wide)
    cpu = LowRank(mean.cpu(), W.cpu(), d.cpu())
    cpu.log_prob(x.cpu())
    assert "CPU" in zs.explain(cpu)
