"""MultivariateNormalCholesky through the public interface, on both back-ends (``vdev``: the torch restatement of
tests/mvn_host.py on the host, the kernels of include/zs_mvn.h on the GPU).  See tests/README_mvn.md."""
import inspect
import math

import pytest
import torch
import torch.distributions as td

import zhusuan as zs
from zhusuan import distributions as D_
from zhusuan.distributions import MultivariateNormalCholesky as MVN
from zhusuan.framework.bn import BayesianNet
from zhusuan.variational.elbo import ELBO
from zhusuan.variational.importance_weighted_objective import ImportanceWeightedObjective

import host_backend
import host_routing
import mvn_host
from mvn_host import vdev  # noqa: F401
from truth import gen, held_to_the_rule, seed_all

F32, F64 = torch.float32, torch.float64


def rand_mean(shape, seed, dev="cpu", dtype=F32):
    return (3.0 * torch.randn(shape, generator=gen(seed), dtype=F64)).to(dtype).to(dev)


def rand_tril(batch, D, seed, dev="cpu", dtype=F32):
    """diagonal U[0.5, 2], strict lower part N(0, 1) 0.5 / sqrt(D), zeros above"""
    g = gen(seed)
    L = torch.tril(torch.randn(tuple(batch) + (D, D), generator=g, dtype=F64) * 0.5 / math.sqrt(D), -1)
    L = L + torch.diag_embed(0.5 + 1.5 * torch.rand(tuple(batch) + (D,), generator=g, dtype=F64))
    return L.to(dtype).to(dev)


def torch_mvn(mean, tril):
    batch = torch.broadcast_shapes(mean.shape[:-1], tril.shape[:-2])
    D = mean.shape[-1]
    return td.MultivariateNormal(mean.expand(batch + (D,)), scale_tril=tril.expand(batch + (D, D)), validate_args=False)


# ------------------------------------------------------------------------------------------------ interface
def test_import_forms_signature_and_defaults():
    import zhusuan.distributions.multivariate as m
    assert m.MultivariateNormalCholesky is MVN and 'MultivariateNormalCholesky' in D_.__all__
    assert zs.distributions.MultivariateNormalCholesky is MVN
    p = inspect.signature(MVN.__init__).parameters
    assert list(p)[:8] == ['self', 'mean', 'cov_tril', 'dtype', 'is_reparameterized', 'use_path_derivative', 'group_ndims', 'device']
    assert p['dtype'].default is None and p['is_reparameterized'].default is True and p['use_path_derivative'].default is False
    assert p['group_ndims'].default == 0 and p['device'].default is None
    q = inspect.signature(BayesianNet.multivariate_normal_cholesky).parameters
    assert list(q)[1:4] == ['name', 'mean', 'cov_tril'] and q['n_samples'].default is None and q['group_ndims'].default == 0
    assert MVN._event_ndims == 1 and MVN._nonreparam_draw_has_zero_grad is True


def test_import_zhusuan_does_not_load_the_library():
    import subprocess
    import sys
    from conftest import PKG_ROOT
    code = ("import sys; sys.path.insert(0, %r); import zhusuan; from zhusuan import _mvn_hip; "
            "from zhusuan.distributions import MultivariateNormalCholesky; assert _mvn_hip._LIB is None; print('lazy')" % PKG_ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "lazy" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("mshape", [(4,), (3, 4), (3, 2, 4)])
@pytest.mark.parametrize("full_tril", [False, True])
def test_shapes_dtypes_and_properties(vdev, mshape, full_tril):
    D = 4
    mean = rand_mean(mshape, 1, vdev)
    tril = rand_tril(mshape[:-1] if full_tril else (), D, 2, vdev)
    d = MVN(mean, tril)
    batch = mshape[:-1]
    assert d.mean is not None and d.cov_tril is not None and tuple(d.batch_shape) == batch
    assert d.is_continuous and d.is_reparameterized and d.dtype == F32
    for n, lead in ((None, ()), (1, ()), (5, (5,))):
        z = d.sample(n)
        assert tuple(z.shape) == lead + batch + (D,) and z.dtype == F32 and z.device.type == vdev.type
        lp = d.log_prob(z)
        assert tuple(lp.shape) == lead + batch and lp.dtype == F32
        lp2 = d.log_prob(z.clone())
        assert torch.allclose(lp, lp2, rtol=1e-5, atol=1e-4)
    if len(batch) >= 1:
        dg = MVN(mean, tril, group_ndims=1)
        z = dg.sample(5)
        assert tuple(dg.log_prob(z).shape) == ((5,) + batch)[:-1] and tuple(dg.log_prob(z.clone()).shape) == ((5,) + batch)[:-1]
        assert torch.allclose(dg.log_prob(z), d.log_prob(z.clone()).sum(-1), rtol=1e-5, atol=1e-4)


def test_tril_batch_broadcasts_over_the_mean(vdev):
    mean, tril = rand_mean((4,), 3, vdev), rand_tril((3, 2), 4, 4, vdev)
    d = MVN(mean, tril)
    assert tuple(d.batch_shape) == (3, 2) and tuple(d.sample(2).shape) == (2, 3, 2, 4)
    want = torch_mvn(mean.cpu().double(), tril.cpu().double()).log_prob(torch.zeros(4, dtype=F64))
    assert float((d.log_prob(torch.zeros(4, device=vdev)).cpu().double() - want).abs().max()) < 1e-4


def test_float64(vdev):
    d = MVN(rand_mean((3, 4), 5, vdev, F64), rand_tril((3,), 4, 6, vdev, F64))
    z = d.sample(2)
    assert z.dtype == F64 and d.log_prob(z).dtype == F64 and d.log_prob(z.clone()).dtype == F64


def test_errors(vdev):
    mean, tril = rand_mean((3, 4), 7, vdev), rand_tril((3,), 4, 8, vdev)
    with pytest.raises(ValueError):
        MVN(torch.tensor(1.0, device=vdev), tril)
    with pytest.raises(ValueError):
        MVN(mean, rand_tril((3,), 5, 8, vdev))
    with pytest.raises(ValueError):
        MVN(mean, tril[..., 0])
    with pytest.raises(ValueError):
        MVN(mean, tril[:, :3])
    with pytest.raises(ValueError):
        MVN(mean, rand_tril((2,), 4, 8, vdev))
    with pytest.raises(ValueError):
        MVN(mean, tril, group_ndims=-1)
    with pytest.raises(NotImplementedError):
        MVN(mean, tril, use_path_derivative=True)
    with pytest.raises(TypeError):
        MVN(mean, tril.double())
    with pytest.raises(ValueError):
        MVN(mean, tril).log_prob(torch.zeros(3, 5, device=vdev))
    with pytest.raises(RuntimeError):
        MVN(mean, tril).log_prob(None)
    with pytest.raises(TypeError):
        MVN(mean, tril).sample(2.5)


def test_given_values_broadcast_against_the_batch_shape(vdev):
    mean, tril = rand_mean((3, 2, 4), 9, vdev), rand_tril((3, 2), 4, 10, vdev)
    ref = torch_mvn(mean.cpu().double(), tril.cpu().double())
    d = MVN(mean, tril)
    for shape in ((4,), (2, 4), (3, 1, 4), (7, 3, 2, 4), (2, 5, 1, 2, 4)):
        v = torch.randn(shape, generator=gen(11))
        lp = d.log_prob(v.to(vdev))
        want = ref.log_prob(v.double())
        assert tuple(lp.shape) == tuple(want.shape)
        assert float((lp.cpu().double() - want).abs().max()) < 1e-4 * (1 + float(want.abs().max()))
    # few rows and many observations: presented to the kernels as rows of one particle
    d1 = MVN(rand_mean((4,), 12, vdev), rand_tril((), 4, 13, vdev))
    v = torch.randn(40, 4, generator=gen(14))
    want = torch_mvn(d1.mean.cpu().double(), d1.cov_tril.cpu().double()).log_prob(v.double())
    with mvn_host.recording() as calls:
        assert float((d1.log_prob(v.to(vdev)).cpu().double() - want).abs().max()) < 1e-4
    assert [(c.name, c.args[2], c.args[1]) for c in calls] == [("logprob", 1, (40, 4, 4))]          # (name, K, cov_tril's shape)


def test_the_upper_triangle_is_not_read(vdev):
    mean, tril = rand_mean((3, 4), 15, vdev), rand_tril((3,), 4, 16, vdev)
    dirty = tril + torch.triu(torch.full_like(tril, float("nan")), 1)
    x = torch.randn(2, 3, 4, generator=gen(17)).to(vdev)
    eps = torch.randn(2, 3, 4, generator=gen(18))
    a, b = MVN(mean, tril), MVN(mean, dirty)
    assert torch.equal(a.log_prob(x), b.log_prob(x))
    with zs.inject_epsilon([eps, eps]):
        assert torch.equal(a.sample(2), b.sample(2))


def test_there_is_no_cpu_fallback():
    mvn_host.uninstall()
    host_backend.uninstall()
    d = MVN(torch.zeros(3, 4), torch.eye(4))
    with pytest.raises(RuntimeError):
        d.sample(2)
    with pytest.raises(RuntimeError):
        d.log_prob(torch.zeros(3, 4))


# ------------------------------------------------------------------------------------------------ against torch.distributions
@pytest.mark.parametrize("D", [1, 3, 10, 64])
def test_log_prob_against_torch_distributions(vdev, D):
    """Within 4 x the float32-vs-float64 distance of torch.distributions.MultivariateNormal(loc, scale_tril=) itself."""
    B, K = 6, 4
    mean, tril = rand_mean((B, D), 20 + D), rand_tril((B,), D, 30 + D)
    v = mean[None] + 2.0 * torch.randn(K, B, D, generator=gen(40 + D))
    want = torch_mvn(mean.double(), tril.double()).log_prob(v.double())
    own32 = torch_mvn(mean, tril).log_prob(v).double()
    dist = float((own32 - want).abs().max())
    got = MVN(mean.to(vdev), tril.to(vdev)).log_prob(v.to(vdev)).cpu().double()
    err = float((got - want).abs().max())
    print("D=%d: error %.3e, torch's own float32 distance %.3e" % (D, err, dist))
    assert err <= 4 * dist, (err, dist)


GRAD_WORST = {}


def unpack_lower(flat, D):
    """[..., D (D + 1) / 2] -> [..., D, D] with the entries on the lower triangle (row-major) and zeros above"""
    idx = torch.tril_indices(D, D)
    scatter = torch.zeros(flat.shape[-1], D * D, dtype=flat.dtype, device=flat.device)
    scatter[torch.arange(flat.shape[-1]), (idx[0] * D + idx[1])] = 1
    return (flat @ scatter).reshape(tuple(flat.shape[:-1]) + (D, D))


def _check_grads(name, got, t32, t64):
    held_to_the_rule(name, zip(("d/dmean", "d/dcov_tril", "d/dvalue"), got, t32, t64), GRAD_WORST)


@pytest.mark.parametrize("D", [1, 3, 10])
def test_gradients_against_float64_autograd(vdev, D):
    """With respect to mean, cov_tril and the value, and of the draw with its density reparameterised and not, against float64
    autograd of the torch formulas within 16 x their own float32-vs-float64 distance (the suite's rule for gradients).  The
    largest multiple seen on the MI355X is recorded in tests/README_mvn.md."""
    B, K = 5, 3
    mean, tril = rand_mean((B, D), 50 + D), rand_tril((B,), D, 60 + D)
    v = mean[None] + 2.0 * torch.randn(K, B, D, generator=gen(70 + D))
    g = torch.randn(K, B, generator=gen(71 + D))
    gz = torch.randn(K, B, D, generator=gen(72 + D))
    eps = torch.randn(K, B, D, generator=gen(73 + D))

    def given(dtype, dev, dist_of):
        m0, t0 = mean.to(dtype).to(dev).requires_grad_(True), tril.to(dtype).to(dev).requires_grad_(True)
        v0 = v.to(dtype).to(dev).requires_grad_(True)
        return [torch.tril(x) if i == 1 else x for i, x in
                enumerate(torch.autograd.grad(dist_of(m0, t0).log_prob(v0), [m0, t0, v0], g.to(dtype).to(dev)))]

    _check_grads("log_prob", given(F32, vdev, MVN), given(F32, "cpu", torch_mvn), given(F64, "cpu", torch_mvn))

    def drawn(dtype, dev, ours, reparam):
        m0, t0 = mean.to(dtype).to(dev).requires_grad_(True), tril.to(dtype).to(dev).requires_grad_(True)
        e = eps.to(dtype)
        if ours:
            d = MVN(m0, t0, is_reparameterized=reparam)
            with zs.inject_epsilon([e]):
                z = d.sample(K)
            assert z.requires_grad == reparam
            lp = d.log_prob(z)
        else:
            z = m0 + (torch.tril(t0) @ e[..., None])[..., 0]
            z = z if reparam else z.detach()
            lp = torch_mvn(m0, t0).log_prob(z)
        loss = (g.to(dtype).to(dev) * lp).sum() + ((gz.to(dtype).to(dev) * z).sum() if reparam else 0.0)
        gm, gt = torch.autograd.grad(loss, [m0, t0])
        return [gm, torch.tril(gt)]

    for reparam in (True, False):
        _check_grads("draw (reparameterised)" if reparam else "draw (detached)", drawn(F32, vdev, True, reparam),
                     drawn(F32, "cpu", False, reparam), drawn(F64, "cpu", False, reparam))
    print("largest multiples: %s" % sorted(GRAD_WORST.items()))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 3, 17])
def test_gradcheck_of_the_float64_functions(D):
    from zhusuan.distributions import _mvn_functions as F
    dev = torch.device("cuda:0")
    K, R = 2, 3
    mean = rand_mean((R, D), 80 + D, dev, F64).requires_grad_(True)
    # gradcheck perturbs every entry: the Function reads (and differentiates) the lower triangle only
    low = rand_tril((R,), D, 81 + D, dev, F64)
    idx = torch.tril_indices(D, D).to(dev)
    packed = low[:, idx[0], idx[1]].clone().requires_grad_(True)

    def unpack(p):
        return unpack_lower(p, D)
    eps = torch.randn(K, R, D, dtype=F64, generator=gen(82 + D)).to(dev)
    x = (mean.detach()[None] + eps).clone().requires_grad_(True)
    kw = dict(eps=1e-6, atol=1e-6, rtol=1e-5, nondet_tol=0.0)
    assert torch.autograd.gradcheck(lambda m, p: F.MvnSampleLogProb.apply(m, unpack(p), eps, 0, 0, None, K, True), (mean, packed), **kw)
    assert torch.autograd.gradcheck(lambda m, p, v: F.MvnLogProb.apply(m, unpack(p), v, K), (mean, packed, x), **kw)
    # The detached draw is no function of its inputs that finite differences could follow (moving mean moves z with it and leaves
    # lp where it was): its gradient is the density's direct dependence, i.e. that of the Function checked above at the fixed z.
    z, lp = F.MvnSampleLogProb.apply(mean, unpack(packed), eps, 0, 0, None, K, False)
    assert not z.requires_grad
    g = torch.randn(K, R, dtype=F64, generator=gen(83 + D)).to(dev)
    got = torch.autograd.grad(lp, (mean, packed), g)
    want = torch.autograd.grad(F.MvnLogProb.apply(mean, unpack(packed), z, K), (mean, packed), g)
    for a, b in zip(got, want):
        assert float((a - b).abs().max()) <= 1e-11 * (1 + float(b.abs().max()))


# ------------------------------------------------------------------------------------------------ launches and streams
def test_own_draw_then_log_prob_is_one_launch_each_way(vdev):
    """Counted through the record of the binding's calls, on both back-ends."""
    with mvn_host.recording() as calls:
        mean = rand_mean((4, 3, 6), 90, vdev).requires_grad_(True)
        tril = rand_tril((4, 3), 6, 91, vdev).requires_grad_(True)
        d = MVN(mean, tril, group_ndims=1)
        z = d.sample(5)
        lp = d.log_prob(z)
        lp0 = d._log_prob_sum(None, 0)
        assert tuple(lp.shape) == (5, 4) and tuple(lp0.shape) == (5, 4, 3)
        assert [c.name for c in calls] == ["sample_logprob"]
        (lp.sum() + z.sum()).backward()
        assert [c.name for c in calls] == ["sample_logprob", "sample_logprob_bwd"]
        assert calls[0].kwargs["call"] == calls[1].kwargs["call"]          # the backward regenerates the forward's noise
        assert zs.explain(d).startswith("V1") and "one launch" in zs.explain(d) and d.last_path["why"] is None
        d.log_prob(z.detach().clone())
        assert [c.name for c in calls][2:] == ["logprob"] and zs.explain(d).startswith("V2")
        # an output that never entered the loss costs no backward launch and no dense zero gradient
        n = len(calls)
        d2 = MVN(mean, tril)
        z2 = d2.sample(3)
        (z2 * z2).sum().backward()          # the draw alone
        assert len(calls) == n + 2 and calls[-1].name == "sample_logprob_bwd"
        d3 = MVN(mean, tril, is_reparameterized=False)
        z3 = d3.sample(3)
        assert not z3.requires_grad and d3.log_prob(z3).requires_grad
        n = len(calls)
        d4 = MVN(mean.detach(), tril.detach())
        x = torch.randn(3, 4, 3, 6, generator=gen(92)).to(vdev).requires_grad_(True)
        d4.log_prob(x).sum().backward()
        assert [c.name for c in calls][n:] == ["logprob", "logprob_bwd"] and x.grad is not None
    print("launches on %s: %s" % (vdev.type, [c.name for c in calls]))


def test_wide_rows_take_the_torch_composition(vdev):
    D, B, K = 65, 3, 2
    mean, tril = rand_mean((B, D), 100), rand_tril((B,), D, 101)
    eps = torch.randn(K, B, D, generator=gen(102))
    d = MVN(mean.to(vdev), tril.to(vdev))
    with mvn_host.recording() as calls:
        with zs.inject_epsilon([eps]):
            z = d.sample(K)
        assert "torch composition" in zs.explain(d) and "64" in d.last_path["why"]
        lp = d.log_prob(z)
        x = mean[None] + torch.randn(K, B, D, generator=gen(103))
        lp2 = d.log_prob(x.to(vdev))
        assert "torch composition" in zs.explain(d) and "solve_triangular" in zs.explain(d)
    assert calls == []
    tz, tlp = mvn_host.reference_sample(mean, tril, eps)
    assert float((z.cpu().double() - tz).abs().max()) < 1e-4 and float((lp.cpu().double() - tlp).abs().max()) < 1e-3
    assert float((lp2.cpu().double() - mvn_host.reference_logprob(mean, tril, x)).abs().max()) < 1e-3
    # a detached wide draw keeps the density's direct dependence on the parameters (what the score-function estimators need)
    m0, t0 = mean.to(vdev).requires_grad_(True), tril.to(vdev).requires_grad_(True)
    dn = MVN(m0, t0, is_reparameterized=False)
    with zs.inject_epsilon([eps]):
        zn = dn.sample(K)
    assert not zn.requires_grad and torch.equal(zn, z.detach())
    gm, gt = torch.autograd.grad(dn.log_prob(zn).sum(), [m0, t0])
    m1, t1 = mean.double().requires_grad_(True), tril.double().requires_grad_(True)
    wm, wt = torch.autograd.grad(torch_mvn(m1, t1).log_prob(tz).sum(), [m1, t1])
    assert float((gm.cpu().double() - wm).abs().max()) < 1e-3 and float((torch.tril(gt).cpu().double() - torch.tril(wt)).abs().max()) < 1e-3
    seed_all(4)
    a = d.sample(K)
    seed_all(4)
    assert torch.equal(a, d.sample(K))


def test_injected_noise_reference_stream_and_seeds_reproduce(vdev):
    mean, tril = rand_mean((4, 6), 110, vdev), rand_tril((4,), 6, 111, vdev)
    eps = torch.randn(3, 4, 6, generator=gen(112))
    d = MVN(mean, tril)
    with zs.inject_epsilon([eps, eps]):
        a, b = d.sample(3), d.sample(3)
    assert torch.equal(a, b)
    assert float((a.cpu().double() - mvn_host.reference_sample(mean.cpu(), tril.cpu(), eps)[0]).abs().max()) < 1e-4
    with pytest.raises(RuntimeError):
        with zs.inject_epsilon([eps[0]]):
            d.sample(3)
    torch.manual_seed(7)
    with zs.reference_rng():
        a = d.sample(3)
    torch.manual_seed(7)
    er = torch.normal(0., 1., size=(3, 4, 6))
    with zs.inject_epsilon([er]):
        b = d.sample(3)
    assert torch.equal(a, b)
    seed_all(9)
    a1, a2 = d.sample(3), d.sample(3)
    seed_all(9)
    b1, b2 = d.sample(3), d.sample(3)
    assert torch.equal(a1, b1) and torch.equal(a2, b2) and not torch.equal(a1, a2)


class Net(BayesianNet):
    def __init__(self, build):
        super().__init__()
        self.build = build

    def forward(self, observed):
        self.observe(observed)
        self.build(self)
        return self


def test_two_nodes_of_one_net_receive_different_calls():
    with host_routing.host(mvn_host.router) as dev, mvn_host.recording() as calls:
        mean, tril = rand_mean((3, 4), 120, dev), rand_tril((3,), 4, 121, dev)

        def build(net):
            net.multivariate_normal_cholesky('a', mean, tril, n_samples=2)
            net.multivariate_normal_cholesky('b', mean, tril, n_samples=2)
        seed_all(5)
        net = Net(build)
        net({})
        a, b = net.nodes['a'].tensor, net.nodes['b'].tensor
        ids = [c.kwargs["call"] for c in calls if c.name == "sample_logprob"]
        # (the factory draws once and the read of .tensor draws again, as in the reference: four draws, four ids)
        assert len(ids) >= 2 and len(set(ids)) == len(ids) and not torch.equal(a, b)


@pytest.mark.gpu
def test_device_rng_reproduces_and_a_graphed_step_draws_fresh_numbers():
    dev = torch.device("cuda:0")
    mean = rand_mean((16, 6), 130, dev).requires_grad_(True)
    tril = rand_tril((16,), 6, 131, dev).requires_grad_(True)
    outs = []
    for _ in range(2):
        rng = zs.DeviceRNG(dev, seed=5)
        with zs.device_rng(rng):
            rng.begin_step()
            outs.append(MVN(mean, tril).sample(4).detach().clone())
    assert torch.equal(outs[0], outs[1])
    rng = zs.DeviceRNG(dev, seed=11)
    held = {}

    def compute():
        rng.begin_step()
        d = MVN(mean, tril)
        z = d.sample(4)
        loss = d.log_prob(z).sum() + (z * z).sum()
        mean.grad = None
        tril.grad = None
        loss.backward()
        held['z'] = z
        return loss.detach()
    step = zs.GraphedStep(compute, rng=rng, warmup=3)
    assert step.captured, step.capture_error
    step()
    torch.cuda.synchronize()
    z1, g1 = held['z'].detach().clone(), tril.grad.clone()
    step()
    torch.cuda.synchronize()
    assert not torch.equal(z1, held['z']) and not torch.equal(g1, tril.grad)


MOMENT_SEED = 2024
MOMENT_L = [[1.0, 0.0, 0.0], [0.5, 0.8, 0.0], [-0.3, 0.4, 1.5]]
MOMENT_MEAN = [1.0, -2.0, 0.5]


def test_moments_of_65536_philox_draws(vdev):
    """n = 65 536 draws at D = 3: every coordinate of the sample mean within 5 sigma_i / sqrt(n), every entry of the sample
    covariance within 6 standard errors of L L^T (the standard error of entry (i, j) is sqrt((S_ii S_jj + S_ij^2) / n)).  The
    seed was chosen on the host back-end, whose stream is the device's bit for bit; observed there: the largest mean deviation is
    recorded in tests/README_mvn.md."""
    n = 65536
    seed_all(MOMENT_SEED)
    L = torch.tensor(MOMENT_L, device=vdev)
    z = MVN(torch.tensor(MOMENT_MEAN, device=vdev), L).sample(n).cpu().double()
    assert tuple(z.shape) == (n, 3)
    S = torch.tensor(MOMENT_L, dtype=F64) @ torch.tensor(MOMENT_L, dtype=F64).T
    dm = (z.mean(0) - torch.tensor(MOMENT_MEAN, dtype=F64)).abs() / (torch.diagonal(S).sqrt() / math.sqrt(n))
    c = z - z.mean(0)
    cov = c.T @ c / (n - 1)
    se = ((torch.diagonal(S)[:, None] * torch.diagonal(S)[None] + S ** 2) / n).sqrt()
    dc = (cov - S).abs() / se
    print("mean deviations in standard errors %s, covariance deviations %s" % (dm.tolist(), dc.tolist()))
    assert bool((dm <= 5).all()) and bool((dc <= 6).all())


# ------------------------------------------------------------------------------------------------ nodes and objectives
def test_bayesian_net_factory_and_log_joint(vdev):
    mean, tril = rand_mean((3, 2, 4), 140, vdev), rand_tril((3, 2), 4, 141, vdev)
    obs = torch.randn(5, 3, 2, 4, generator=gen(142)).to(vdev)

    def build(net):
        net.multivariate_normal_cholesky('a', mean, tril, n_samples=5, group_ndims=1)
        net.stochastic_node('MultivariateNormalCholesky', 'b', mean=mean, cov_tril=tril, n_samples=5, reduce_sum_dims=[-1])
    net = Net(build).to(vdev)
    net({})
    assert tuple(net.nodes['a'].tensor.shape) == (5, 3, 2, 4) and tuple(net.nodes['a'].log_prob().shape) == (5, 3)
    assert tuple(net.nodes['b'].log_prob().shape) == (5, 3) and tuple(net.log_joint().shape) == (5, 3)
    net({'a': obs})
    assert net.nodes['a'].tensor is obs
    want = torch_mvn(mean.cpu().double(), tril.cpu().double()).log_prob(obs.cpu().double()).sum(-1)
    assert float((net.nodes['a'].log_prob().cpu().double() - want).abs().max()) < 1e-3
    assert tuple(net.log_joint().shape) == (5, 3)
    with pytest.raises(ValueError):
        net.multivariate_normal_cholesky(3, mean, tril)


OB, OK_, OD, OX = 3, 5, 4, 6
NTRI = OD * (OD + 1) // 2


def objective_setup(dev, dtype):
    g = gen(150)
    P = dict(enc_m=0.7 * torch.randn(OX, OD, generator=g, dtype=F64), enc_l=0.3 * torch.randn(OX, NTRI, generator=g, dtype=F64),
             dec=0.7 * torch.randn(OD, OX, generator=g, dtype=F64), bias=0.3 * torch.randn(OX, generator=g, dtype=F64))
    P = {k: v.to(dtype).to(dev).requires_grad_(True) for k, v in P.items()}
    x = (torch.rand(OB, OX, generator=g) < 0.5).to(dtype).to(dev)
    return P, x


def assemble(flat):
    """[..., D (D + 1) / 2] -> lower-triangular [..., D, D] with an exp diagonal"""
    L = unpack_lower(flat, OD)
    dg = torch.diagonal(L, dim1=-2, dim2=-1)
    return L - torch.diag_embed(dg) + torch.diag_embed(torch.exp(dg))


MODES = {"sgvb": ("elbo", "sgvb", True), "reinforce": ("elbo", "reinforce", False), "iw_sgvb": ("iw", "sgvb", True),
         "vimco": ("iw", "vimco", False)}


def make_objective(kind, estimator, gen_net, var_net):
    if kind == "iw":
        return ImportanceWeightedObjective(gen_net, var_net, axis=0, estimator=estimator)
    return ELBO(gen_net, var_net, estimator=estimator)


def zs_objective(mode, dev, P, x, eps):
    kind, estimator, reparam = MODES[mode]
    K = OK_ if kind == "iw" else None

    def q(net):
        net.multivariate_normal_cholesky('z', net.observed['x'] @ P['enc_m'], assemble(net.observed['x'] @ P['enc_l']), n_samples=K,
                                         is_reparameterized=reparam)

    def p(net):
        z = net.normal('z', mean=torch.zeros(OB, OD, dtype=x.dtype, device=dev), std=torch.ones(OB, OD, dtype=x.dtype, device=dev),
                       n_samples=K, group_ndims=1)
        net.bernoulli('x', logits=z @ P['dec'] + P['bias'], group_ndims=1)
    obj = make_objective(kind, estimator, Net(p).to(dev), Net(q).to(dev)).to(dev)
    with zs.inject_epsilon([eps, eps]):          # the objectives draw every latent twice and use the second draw
        loss = obj({'x': x})
    return loss, torch.autograd.grad(loss, list(P.values()), allow_unused=True)


def torch_objective(mode, dev, dtype, x, eps):
    """The same model with torch.distributions on the CPU in `dtype`; the objectives' own epilogue on (log p, log q)."""
    kind, estimator, reparam = MODES[mode]
    P, _ = objective_setup("cpu", dtype)
    xc = x.detach().cpu().to(dtype)
    mean, L = xc @ P['enc_m'], assemble(xc @ P['enc_l'])
    K = OK_ if kind == "iw" else 1
    e = eps.to(dtype).reshape(K, OB, OD)
    z = mean[None] + (L[None] @ e[..., None])[..., 0]
    if not reparam:
        z = z.detach()
    logq = td.MultivariateNormal(mean, scale_tril=L).log_prob(z)
    logpz = td.Normal(torch.zeros(OB, OD, dtype=dtype), torch.ones(OB, OD, dtype=dtype)).log_prob(z).sum(-1)
    logpx = td.Bernoulli(logits=z @ P['dec'] + P['bias']).log_prob(xc[None].expand(K, OB, OX)).sum(-1)
    logp = logpz + logpx
    if kind != "iw":
        logp, logq = logp[0], logq[0]
    obj = make_objective(kind, estimator, Net(None), Net(None)).to(dev)
    loss = getattr(obj, estimator)(logp.to(dev), logq.to(dev))
    return loss, torch.autograd.grad(loss, list(P.values()), allow_unused=True)


@pytest.mark.parametrize("mode", sorted(MODES))
def test_objectives_over_a_multivariate_normal_latent(vdev, mode):
    """Value and parameter gradients against the same model written with torch.distributions in float64 with the same injected
    eps, within 16 x that model's own float32-vs-float64 distance."""
    K = OK_ if MODES[mode][0] == "iw" else 1
    eps = torch.randn(((K,) if K > 1 else ()) + (OB, OD), generator=gen(151))
    P, x = objective_setup(vdev, F32)
    loss, grads = zs_objective(mode, vdev, P, x, eps)
    l64, g64 = torch_objective(mode, vdev, F64, x, eps)
    l32, g32 = torch_objective(mode, vdev, F32, x, eps)
    pairs = [("loss", loss, l32, l64)] + [(n, a, b, c) for n, a, b, c in zip(P.keys(), grads, g32, g64)]
    for name, a, b, c in pairs:
        assert (a is None) == (c is None), name
    held_to_the_rule(mode, [p for p in pairs if p[1] is not None])
