"""GPConditional and ``BayesianNet.gp_conditional`` (zhusuan/distributions/gp.py): the public interface over the kernels of
include/zs_gp.h.  The truth and the tolerance are those of tests/test_gp_kernel.py; the objective is held to the suite's rule
(16 x the float32 model's own distance from float64)."""
import pytest
import torch
import torch.distributions as td

import zhusuan as zs
from zhusuan.distributions import GPConditional, Normal
from zhusuan.distributions._gp_functions import torch_moments

from kernel_abi import unit
from test_gp_kernel import NAMES, case_inputs, case_truth, defined_moments, evaluate
from truth import gen, held_to_the_rule

F32, F64 = torch.float32, torch.float64


def with_std(fn):
    """(mean, std) of a function that gives (mean, var)"""
    def moments(*p):
        mean, var = fn(*p)
        return mean, torch.sqrt(torch.clamp(var, min=0))
    return moments


def public_moments(dev, dtype, ins):
    """mean, std and the gradients of sum(gmean mean) + sum(gvar std) through the class, in the order NAMES (std in var's place)"""
    ps = [t.to(dtype).to(dev).clone().requires_grad_(True) for t in ins[:6]]
    x, Z, l, a, L, fz = ps
    dist = GPConditional(x, Z, fz, L, l, a.reshape(()))
    loss = (dist.mean * ins[6].to(dtype).to(dev)).sum() + (dist.std * ins[7].to(dtype).to(dev)).sum()
    return dist, dict(zip(NAMES, (dist.mean.detach(), dist.std.detach()) + torch.autograd.grad(loss, ps)))


def std_truth(ins):
    """the truth of public_moments and, per element type, the tolerance of tests/test_gp_kernel.py for it"""
    t = evaluate(with_std(defined_moments), ins, F64)
    tols = {}
    for dtype in (F32, F64):
        comp = evaluate(with_std(torch_moments), ins, dtype)
        tols[dtype] = dict((n, 16 * float((comp[n] - t[n]).abs().max()) + 4 * unit(dtype) * float(t[n].abs().max())) for n in NAMES)
    return t, tols


# ------------------------------------------------------------------------------------------------ no GPU
@pytest.mark.parametrize("N,M,d,K", [(33, 17, 3, 5), (9, 130, 2, 1)])
def test_cpu_tensors_run_the_torch_composition(N, M, d, K):
    """The composition in float64 against the definition: the two differ by float64 rounding only (1e-9 relative)."""
    assert 'GPConditional' in zs.distributions.__all__ and hasattr(zs.framework.bn.BayesianNet, 'gp_conditional')
    ins = case_inputs(N, M, d, K)
    t, c = evaluate(with_std(defined_moments), ins, F64), evaluate(with_std(torch_moments), ins, F64)
    dist, got = public_moments("cpu", F64, ins)
    for n in NAMES:
        assert float((c[n] - t[n]).abs().max()) <= 1e-9 * float(t[n].abs().max()), n
        assert float((got[n].reshape(t[n].shape) - t[n]).abs().max()) <= 1e-9 * float(t[n].abs().max()), n
    assert tuple(dist.batch_shape) == (K, N) and tuple(dist.std.shape) == (N,)
    assert torch.equal(dist.std, torch.sqrt(torch.clamp(dist.var, min=0)))
    assert dist.last_path["path"].startswith("torch composition") and "CPU" in zs.explain(dist)
    x, Z, l, a, L, fz = ins[:6]
    assert tuple(GPConditional(x, Z, fz[0], L, l, a).batch_shape) == (N,)
    tril = GPConditional.gram_tril(Z, l, a, jitter=0.1 * float(a) ** 2)
    assert float((tril - L).abs().max()) <= 1e-6          # (L is the float32 rounding of this factor)
    for bad in (dict(inducing=Z[:, :-1]) if d > 1 else dict(x=x[0]), dict(f_inducing=fz[:, :-1]), dict(kzz_tril=L[:-1]),
                dict(lengthscale=torch.ones(d + 1, dtype=F64)), dict(amplitude=torch.ones(2, dtype=F64))):
        kw = dict(x=x, inducing=Z, f_inducing=fz, kzz_tril=L, lengthscale=l, amplitude=a)
        kw.update(bad)
        with pytest.raises(ValueError):
            GPConditional(**kw)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_draws_and_densities_are_the_normal_on_the_moments():
    x, Z, l, a, L, fz = (t.to(F32).to("cuda:0") for t in case_inputs(17, 5, 2, 3)[:6])
    dist = GPConditional(x, Z, fz, L, l, a, group_ndims=1)
    ref = Normal(dist.mean, std=dist.std, group_ndims=1)
    eps = torch.randn(3, 17).to("cuda:0")
    with zs.inject_epsilon([eps, eps]):
        z, zr = dist.sample(), ref.sample()
    assert tuple(z.shape) == (3, 17) and torch.equal(z, zr)
    assert torch.equal(dist.log_prob(None), ref.log_prob(zr)) and tuple(dist.log_prob(zr + 1).shape) == (3,)
    assert torch.equal(dist.log_prob(zr + 1), ref.log_prob(zr + 1))


@pytest.mark.gpu
@pytest.mark.parametrize("N,M,d,K", [(33, 17, 3, 5), (150, 64, 5, 17)])
def test_moments_and_gradients_on_the_kernels(N, M, d, K):
    ins = case_truth(N, M, d, K, False)[0]
    t, tols = std_truth(ins)
    for dtype in (F32, F64):
        dist, got = public_moments(torch.device("cuda:0"), dtype, ins)
        assert "zs_gp_moments" in zs.explain(dist) and dist.last_path["why"] is None
        for n in NAMES:
            err = float((got[n].cpu().double().reshape(t[n].shape) - t[n]).abs().max())
            assert err <= tols[dtype][n], (n, dtype, err / tols[dtype][n])


@pytest.mark.gpu
def test_routing_named_in_explain():
    dev = torch.device("cuda:0")
    ins = case_inputs(9, 130, 2, 3)
    x, Z, l, a, L, fz = (t.to(F32).to(dev) for t in ins[:6])
    wide = GPConditional(x, Z, fz, L, l, a)          # M = 130
    t, tols = std_truth(ins)
    for name, got in (("mean", wide.mean), ("var", wide.std)):
        assert float((got.cpu().double() - t[name]).abs().max()) <= tols[F32][name], name
    assert wide.last_path["path"].startswith("torch composition") and "zs_gp_max_inducing" in zs.explain(wide) and "128" in zs.explain(wide)
    small = GPConditional(x, Z[:16], fz[:, :16], GPConditional.gram_tril(Z[:16], l, a, jitter=0.1), l, a)
    assert tuple(small.sample(2).shape) == (2, 3, 9) and "zs_gp_prepare" in zs.explain(small)
    cpu = GPConditional(*(t.cpu() for t in (x, Z, fz, L, l, a)))
    assert tuple(cpu.mean.shape) == (3, 9) and "CPU" in zs.explain(cpu)


# the examples/svgp.py model at its smallest size: 17 inducing inputs (two tiles), 33 inputs, five particles
ON, OM, OK_ = 33, 17, 5
JITTER = 0.1          # as in tests/test_gp_kernel.py: var >= 0.05 a^2, so the rule measures the kernels, not the conditioning of L


def svgp_setup(dev, dtype):
    from examples import svgp
    g = gen(520)
    x, y = svgp.synthetic(ON, 1, g)
    P = {k: v.to(F64) + 0.1 * torch.randn(v.shape, generator=g, dtype=F64) for k, v in svgp.init_params(x, OM, g).items()}
    return svgp, {k: v.to(dtype).to(dev).requires_grad_(True) for k, v in P.items()}, x.to(dtype).to(dev), y.to(dtype).to(dev)


def torch_svgp(dtype, eps):
    """The same model with torch.distributions on the CPU in `dtype`, drawn as the objective draws: the variational net runs on
    the first draw of f_Z, every latent is drawn again, and the second draws are the ones scored."""
    svgp, P, x, y = svgp_setup("cpu", dtype)
    e1, _, e3, e4 = (e.to(dtype) for e in eps)
    length, amp, noise = torch.exp(P['log_length']), torch.exp(P['log_amp']), torch.exp(P['log_noise'])
    L, Lq = GPConditional.gram_tril(P['inducing'], length, amp, jitter=JITTER * amp ** 2), svgp.q_tril(P['q_raw'])
    fz1, fz2 = P['q_mean'] + e1 @ Lq.T, P['q_mean'] + e3 @ Lq.T
    (m1, std), (m2, _) = (with_std(defined_moments)(x, P['inducing'], length, amp, L, fz) for fz in (fz1, fz2))
    f = m1 + std * e4
    logq = td.MultivariateNormal(P['q_mean'], scale_tril=Lq).log_prob(fz2) + td.Normal(m1, std).log_prob(f).sum(-1)
    logp = (td.MultivariateNormal(torch.zeros(OM, dtype=dtype), scale_tril=L).log_prob(fz2) + td.Normal(m2, std).log_prob(f).sum(-1)
            + td.Normal(f, noise).log_prob(y).sum(-1))
    loss = -(logp - logq).mean()
    return loss, torch.autograd.grad(loss, list(P.values()))


@pytest.mark.gpu
def test_one_sgvb_step_of_the_svgp_model():
    """Value and parameter gradients against the same model written with torch.distributions in float64 with the same injected
    eps, within 16 x that model's own float32-vs-float64 distance."""
    dev = torch.device("cuda:0")
    g = gen(521)
    eps = [torch.randn(OK_, n, generator=g) for n in (OM, ON, OM, ON)]          # f_Z and f, each drawn twice
    svgp, P, x, y = svgp_setup(dev, F32)
    objective = svgp.build(P, x, particles=OK_, jitter=JITTER, device=dev)
    with zs.inject_epsilon(eps):
        loss = objective({'y': y})
    grads = torch.autograd.grad(loss, list(P.values()))
    for net in (objective.variational, objective.generator):
        assert "zs_gp_moments" in zs.explain(net.nodes['f'].dist) and net.nodes['f'].dist.last_path["why"] is None
    l64, g64 = torch_svgp(F64, eps)
    l32, g32 = torch_svgp(F32, eps)
    held_to_the_rule("sgvb", [("loss", loss, l32, l64)] + list(zip(P.keys(), grads, g32, g64)))
