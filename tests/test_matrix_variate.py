"""MatrixVariateNormalCholesky and ``BayesianNet.matrix_variate_normal_cholesky`` (zhusuan/distributions/matrix_variate.py): the
public interface over the kernels of include/zs_matvar.h.  The truth and the bounds of the GPU tests are those of
tests/test_matvar_kernel.py; the objectives are held to the suite's rule (16 x the float32 model's own distance from float64)."""
import inspect
import os
import subprocess
import sys

import pytest
import torch
import torch.distributions as td

import zhusuan as zs
from zhusuan.distributions import MatrixVariateNormalCholesky as MVN
from zhusuan.framework.bn import BayesianNet, name_mapping
from zhusuan.variational.elbo import ELBO
from zhusuan.variational.importance_weighted_objective import ImportanceWeightedObjective

import host_routing
from test_matvar_kernel import bounds, case_inputs, low, truth
from truth import gen, held_to_the_rule

F32, F64 = torch.float32, torch.float64
CALLS = host_routing.Router("zhusuan._matvar_hip", dict.fromkeys(["sample_logprob", "sample_logprob_bwd", "logprob", "logprob_bwd"]))


class Net(BayesianNet):
    def __init__(self, build):
        super().__init__()
        self.build = build

    def forward(self, observed):
        self.observe(observed)
        self.build(self)
        return self


def kron_tril(U, V):
    """the Cholesky factor of kron(U U^T, V V^T) for batched factors: vec stacks the rows of the event"""
    n, p = U.shape[-1], V.shape[-1]
    return (U[..., :, None, :, None] * V[..., None, :, None, :]).reshape(U.shape[:-2] + (n * p, n * p))


# ------------------------------------------------------------------------------------------------ interface (no GPU)
def test_import_forms_signature_and_registration():
    import zhusuan.distributions.matrix_variate as m
    assert m.MatrixVariateNormalCholesky is MVN is zs.distributions.MatrixVariateNormalCholesky is name_mapping['MatrixVariateNormalCholesky']
    assert 'MatrixVariateNormalCholesky' in zs.distributions.__all__ and MVN._event_ndims == 2
    assert list(inspect.signature(MVN.__init__).parameters)[:9] == ['self', 'mean', 'u_tril', 'v_tril', 'dtype', 'is_reparameterized',
                                                                    'use_path_derivative', 'group_ndims', 'device']
    assert list(inspect.signature(BayesianNet.matrix_variate_normal_cholesky).parameters)[:5] == ['self', 'name', 'mean', 'u_tril', 'v_tril']


def test_import_loads_neither_the_binding_nor_the_library():
    code = ("import sys, zhusuan; from zhusuan.distributions import MatrixVariateNormalCholesky; "
            "assert 'zhusuan._matvar_hip' not in sys.modules; from zhusuan import _matvar_hip; assert _matvar_hip._LIB is None")
    pkg_root = os.path.dirname(os.path.dirname(os.path.abspath(zs.__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=pkg_root, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


def test_shapes_and_errors():
    eye = torch.eye
    d = MVN(torch.zeros(2, 1, 3, 4), eye(3).expand(5, 3, 3), eye(4), device="cpu")
    assert tuple(d.batch_shape) == (2, 5) and d.dtype == F32 and d.mean.shape == (2, 1, 3, 4) and d.u_tril.shape == (5, 3, 3) and d.v_tril.shape == (4, 4)
    assert tuple(d.sample().shape) == (2, 5, 3, 4) and tuple(d.sample(7).shape) == (7, 2, 5, 3, 4) and tuple(d.log_prob(torch.zeros(7, 2, 5, 3, 4)).shape) == (7, 2, 5)
    assert tuple(MVN(torch.zeros(2, 5, 3, 4), eye(3), eye(4), group_ndims=1, device="cpu").log_prob(torch.zeros(3, 4)).shape) == (2,)
    with pytest.raises(ValueError, match=r"u_tril must have shape \[\.\.\., 3, 3\].*\(4, 4\)"):
        MVN(torch.zeros(3, 4), eye(4), eye(4), device="cpu")
    with pytest.raises(ValueError, match=r"v_tril must have shape \[\.\.\., 4, 4\].*\(3, 3\)"):
        MVN(torch.zeros(3, 4), eye(3), eye(3), device="cpu")
    with pytest.raises(ValueError, match=r"do not broadcast"):
        MVN(torch.zeros(2, 3, 4), eye(3).expand(3, 3, 3), eye(4), device="cpu")
    with pytest.raises(ValueError, match=r"\[3, 4\].*\(4, 3\)"):
        d.log_prob(torch.zeros(4, 3))
    with pytest.raises(NotImplementedError, match="use_path_derivative"):
        MVN(torch.zeros(3, 4), eye(3), eye(4), use_path_derivative=True, device="cpu")


@pytest.mark.parametrize("n,p", [(3, 4), (17, 5)])
def test_cpu_tensors_run_the_torch_composition_with_row_major_kronecker_covariance(n, p):
    d = case_inputs(n, p, 2, 3)
    leaves = [d[k].clone().requires_grad_(True) for k in ("mean", "U", "V", "x")]          # (NaN above the diagonals: never read)
    dist = MVN(*leaves[:3])
    got = dist.log_prob(leaves[3])
    assert dist.last_path["path"].startswith("torch composition") and "CPU" in zs.explain(dist)
    ref = [d["mean"].clone().requires_grad_(True), low(d["U"]).requires_grad_(True), low(d["V"]).requires_grad_(True), d["x"].clone().requires_grad_(True)]
    want = td.MultivariateNormal(ref[0].reshape(2, n * p), scale_tril=kron_tril(ref[1], ref[2])).log_prob(ref[3].reshape(3, 2, n * p))
    swapped = td.MultivariateNormal(ref[0].reshape(2, n * p), scale_tril=kron_tril(ref[2], ref[1])).log_prob(ref[3].reshape(3, 2, n * p))
    scale = float(want.detach().abs().max())
    assert float((got - want).detach().abs().max()) <= 1e-9 * scale and float((got - swapped).detach().abs().max()) > 1e-3
    for i, (a, b) in enumerate(zip(torch.autograd.grad(got, leaves, d["g"]), torch.autograd.grad(want, ref, d["g"]))):
        a, b = (torch.tril(a), torch.tril(b)) if i in (1, 2) else (a, b)          # the reference's leaf is dense: its lower triangle
        assert float((a - b).abs().max()) <= 1e-8 * (1 + float(b.abs().max()))
    z = dist.sample(3)          # the draw's own density is that of the value
    assert float((dist.log_prob(z) - dist.log_prob(z.detach().clone())).detach().abs().max()) <= 1e-9 * scale


# ------------------------------------------------------------------------------------------------ on the kernels
def check(name, got, want, tol):
    err = (got.detach().cpu().to(F64).reshape(want.shape) - want).abs()
    print("%s: worst error / tolerance = %.3f" % (name, float((err / tol).max())))
    assert bool((err <= tol).all()), name


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64])
def test_nodes_of_a_bayesian_net_run_the_kernels(dtype):
    n, p, B, K = 5, 4, 3, 5
    d = case_inputs(n, p, B, K)
    dev = torch.device("cuda:0")
    g, gz = d["g"].to(dev, dtype), d["gz"].to(dev, dtype)

    def node(observed, reparam=True):
        leaves = [d[k].to(dev, dtype).requires_grad_(True) for k in ("mean", "U", "V")]
        net = Net(lambda net: net.matrix_variate_normal_cholesky("w", *leaves, n_samples=K, is_reparameterized=reparam)).to(dev)
        with zs.inject_epsilon([] if observed else [d["eps"].to(dtype)]):          # (an observed node draws nothing)
            net(observed)
        return net, leaves

    t, tol = truth(d), bounds(dtype, d, truth(d), K)
    x = d["x"].to(dev, dtype).requires_grad_(True)
    net, leaves = node({"w": x})
    lp = net.log_joint()
    assert net.nodes["w"].dist.last_path["path"].startswith("M2 zs_matvar_logprob") and net.nodes["w"].dist.last_path["why"] is None
    for k, got in zip(("lp2", "gm2", "gu2", "gv2", "gx"), (lp,) + torch.autograd.grad(lp, leaves + [x], g)):
        check("observed " + k, got, t[k], tol[k])
    net, leaves = node({})
    z, lp = net.nodes["w"].dist.sample_cache, net.log_joint()          # (node.tensor would draw afresh)
    assert net.nodes["w"].dist.last_path["path"].startswith("M1 zs_matvar_sample_logprob") and z.requires_grad
    for k, got in zip(("z", "lp1", "gm1", "gu1", "gv1"), (z, lp) + torch.autograd.grad((g * lp).sum() + (gz * z).sum(), leaves)):
        check("drawn " + k, got, t[k], tol[k])
    net, leaves = node({}, reparam=False)          # the detached draw: the density's direct dependence, at the fixed z
    z, lp = net.nodes["w"].dist.sample_cache, net.log_joint()
    assert not z.requires_grad
    zd = z.cpu().to(F64)
    tz, tolz = truth(d, zd), bounds(dtype, d, truth(d, zd), K, zd)
    for k, got in zip(("gm2", "gu2", "gv2"), torch.autograd.grad(lp, leaves, g)):
        check("detached " + k, got, tz[k], tolz[k])


@pytest.mark.gpu
def test_launches_and_routing():
    dev = torch.device("cuda:0")
    d = case_inputs(5, 4, 3, 5)
    leaves = [d[k].to(dev, F32).requires_grad_(True) for k in ("mean", "U", "V")]
    with CALLS.recording() as calls:
        dist = MVN(*leaves)
        z = dist.sample(5)
        dist.log_prob(z).sum().backward()          # the node's own draw: its density came with it
        assert [c.name for c in calls] == ["sample_logprob", "sample_logprob_bwd"]
        assert all(calls[1].kwargs[k] == calls[0].kwargs[k] for k in ("seed", "call")) and calls[1].kwargs["eps"] is None
        del calls[:]
        wide = MVN(torch.zeros(129, 2, device=dev), torch.eye(129, device=dev), torch.eye(2, device=dev))
        wide.log_prob(wide.sample(2))
        wide.log_prob(torch.zeros(129, 2, device=dev))
        assert calls == [] and wide.last_path["path"].startswith("torch composition") and "128" in zs.explain(wide)
        # 19 observations against one weight matrix: folded into 19 rows of one particle (fold_particles), the same density
        one = MVN(*(leaf.detach()[0] for leaf in leaves))
        x = torch.randn(19, 5, 4, generator=gen(170)).to(dev)
        lp = one.log_prob(x)
        assert [c.name for c in calls] == ["logprob"] and calls[0].args[:5] == ((19, 5, 4), (19, 5, 5), (19, 4, 4), 1, (1, 19, 5, 4))
        want = MVN(*(leaf.detach()[0].cpu().double() for leaf in leaves)).log_prob(x.cpu().double())
        assert tuple(lp.shape) == (19,) and float((lp.cpu().double() - want).abs().max()) <= 1e-4 * float(want.abs().max())
    assert all(leaf.grad is not None and bool(torch.isfinite(torch.tril(leaf.grad)).all()) for leaf in leaves)


OB, OK_, ON, OP, OX = 3, 5, 5, 4, 6
MODES = {"sgvb": ("elbo", "sgvb"), "vimco": ("iw", "vimco")}
WORST = {}


def factor_of(raw):
    dg = torch.diagonal(raw, dim1=-2, dim2=-1)
    return 0.3 * torch.tril(raw, -1) + torch.diag_embed(torch.exp(0.3 * dg))


def objective_setup(dev, dtype):
    g = gen(160)
    P = dict(m=torch.randn(OB, ON, OP, generator=g, dtype=F64), u=torch.randn(OB, ON, ON, generator=g, dtype=F64), v=torch.randn(OP, OP, generator=g, dtype=F64))
    P = {k: v.to(dtype).to(dev).requires_grad_(True) for k, v in P.items()}
    x, y = torch.randn(OB, OX, ON, generator=g, dtype=F64), torch.randn(OB, OX, OP, generator=g, dtype=F64)
    return P, x.to(dtype).to(dev), y.to(dtype).to(dev)


def objective_of(kind, estimator, p, q):
    return ImportanceWeightedObjective(p, q, axis=0, estimator=estimator) if kind == "iw" else ELBO(p, q, estimator=estimator)


def zs_objective(mode, dev, eps):
    kind, estimator = MODES[mode]
    K = OK_ if kind == "iw" else None
    P, x, y = objective_setup(dev, F32)

    def q(net):
        net.matrix_variate_normal_cholesky('w', P['m'], factor_of(P['u']), factor_of(P['v']), n_samples=K, is_reparameterized=estimator == "sgvb")

    def p(net):
        w = net.normal('w', mean=torch.zeros(OB, ON, OP, device=dev), std=torch.ones(OB, ON, OP, device=dev), n_samples=K, group_ndims=2)
        net.normal('y', mean=x @ w, std=torch.ones(OB, OX, OP, device=dev), group_ndims=2)
    obj = objective_of(kind, estimator, Net(p).to(dev), Net(q).to(dev)).to(dev)
    with zs.inject_epsilon([eps, eps]):          # the objectives draw every latent twice and use the second draw
        loss = obj({'y': y})
    return loss, torch.autograd.grad(loss, list(P.values()))


def torch_objective(mode, dev, dtype, eps):
    """The same model with torch.distributions on the CPU in `dtype`; the objectives' own epilogue on (log p, log q)."""
    kind, estimator = MODES[mode]
    P, x, y = objective_setup("cpu", dtype)
    K = OK_ if kind == "iw" else 1
    U, V = factor_of(P['u']), factor_of(P['v'])
    w = P['m'] + U @ eps.to(dtype).reshape(K, OB, ON, OP) @ V.mT
    w = w if estimator == "sgvb" else w.detach()
    logq = td.MultivariateNormal(P['m'].reshape(OB, -1), scale_tril=kron_tril(U, V.expand(OB, OP, OP))).log_prob(w.reshape(K, OB, -1))
    logp = td.Normal(0.0, 1.0).log_prob(w).sum((-1, -2)) + td.Normal(x @ w, 1.0).log_prob(y).sum((-1, -2))
    if kind != "iw":
        logp, logq = logp[0], logq[0]
    obj = objective_of(kind, estimator, Net(None), Net(None)).to(dev)
    loss = getattr(obj, estimator)(logp.to(dev), logq.to(dev))
    return loss, torch.autograd.grad(loss, list(P.values()))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", sorted(MODES))
def test_objectives_over_a_matrix_variate_latent(mode):
    """Value and parameter gradients against the same model written with torch.distributions in float64 with the same injected
    eps, within 16 x that model's own float32-vs-float64 distance; the multiples seen are in tests/README_matvar.md."""
    dev = torch.device("cuda:0")
    K = OK_ if MODES[mode][0] == "iw" else 1
    eps = torch.randn(((K,) if K > 1 else ()) + (OB, ON, OP), generator=gen(161))
    loss, grads = zs_objective(mode, dev, eps)
    l64, g64 = torch_objective(mode, dev, F64, eps)
    l32, g32 = torch_objective(mode, dev, F32, eps)
    held_to_the_rule(mode, [("loss", loss, l32, l64)] + list(zip("muv", grads, g32, g64)), WORST)
    print("largest multiples: %s" % sorted(WORST.items()))
