"""Categorical, OnehotCategorical, ExpConcrete and Concrete through the public interface, on both back-ends (``cdev``: the torch
restatement of tests/cat_host.py on the host, the kernels of include/zs_cat.h on the GPU).  See tests/README_cat.md."""
import inspect

import numpy as np
import pytest
import torch
import torch.distributions as td
from torch.distributions import relaxed_categorical as trc

import zhusuan as zs
from zhusuan import distributions as D
from zhusuan.distributions import Categorical, OnehotCategorical, ExpConcrete, Concrete
from zhusuan.framework.bn import BayesianNet
from zhusuan.variational.elbo import ELBO
from zhusuan.variational.importance_weighted_objective import ImportanceWeightedObjective

import cat_host
import host_backend
from cat_host import cdev  # noqa: F401
from truth import gen, held_to_the_rule, seed_all

F32, F64 = torch.float32, torch.float64
FAMILIES = [Categorical, OnehotCategorical, ExpConcrete, Concrete]


def make(cls, logits, tau=0.7, **kw):
    if cls in (ExpConcrete, Concrete):
        return cls(tau, logits, **kw)
    return cls(logits, **kw)


def rand_logits(shape, seed, dev, dtype=F32):
    g = gen(seed)
    return (1.5 * torch.randn(shape, generator=g, dtype=F64)).to(dtype).to(dev)


def rand_u(shape, seed, dtype=F32):
    g = gen(seed)
    return ((torch.randint(0, 1 << 23, shape, generator=g).double() + 0.5) * 2.0 ** -23).to(dtype)


# ------------------------------------------------------------------------------------------------ interface
def test_import_forms_aliases_signatures_and_defaults():
    import zhusuan.distributions.categorical as c
    import zhusuan.distributions.concrete as k
    assert c.Discrete is Categorical and c.OnehotDiscrete is OnehotCategorical
    assert k.ExpGumbelSoftmax is ExpConcrete and k.GumbelSoftmax is Concrete
    for n in ('Categorical', 'OnehotCategorical', 'Discrete', 'OnehotDiscrete', 'ExpConcrete', 'Concrete', 'ExpGumbelSoftmax',
              'GumbelSoftmax'):
        assert n in D.__all__ and getattr(D, n) is getattr(zs.distributions, n)
    p = inspect.signature(Categorical.__init__).parameters
    assert list(p)[:5] == ['self', 'logits', 'dtype', 'group_ndims', 'device']
    assert p['dtype'].default is None and p['group_ndims'].default == 0 and p['device'].default is None
    p = inspect.signature(ExpConcrete.__init__).parameters
    assert list(p)[:3] == ['self', 'temperature', 'logits'] and p['is_reparameterized'].default is True
    for name, first in (('categorical', ['name', 'logits']), ('onehot_categorical', ['name', 'logits']),
                        ('exp_concrete', ['name', 'temperature', 'logits']), ('concrete', ['name', 'temperature', 'logits'])):
        q = inspect.signature(getattr(BayesianNet, name)).parameters
        assert list(q)[1:1 + len(first)] == first and q['n_samples'].default is None and q['group_ndims'].default == 0
    assert D.Distribution._event_ndims == 0 and Categorical._event_ndims == 0
    assert OnehotCategorical._event_ndims == 1 and ExpConcrete._event_ndims == 1 and Concrete._event_ndims == 1


def test_import_zhusuan_does_not_load_the_library():
    import subprocess
    import sys
    from conftest import PKG_ROOT
    code = ("import sys; sys.path.insert(0, %r); import zhusuan; from zhusuan import _cat_hip; "
            "from zhusuan.distributions import Categorical; assert _cat_hip._LIB is None; print('lazy')" % PKG_ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "lazy" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("cls", FAMILIES)
@pytest.mark.parametrize("shape", [(5,), (3, 5), (3, 2, 5)])
def test_shapes_dtypes_and_properties(cdev, cls, shape):
    lg = rand_logits(shape, 1, cdev)
    d = make(cls, lg)
    assert d.n_categories == 5 and d.logits is not None and tuple(d.batch_shape) == shape[:-1]
    discrete = cls in (Categorical, OnehotCategorical)
    assert d.is_continuous == (not discrete) and d.is_reparameterized == (not discrete) and d._nonreparam_draw_has_zero_grad
    event = () if cls is Categorical else (5,)
    for n, lead in ((None, ()), (1, ()), (5, (5,))):
        z = d.sample(n)
        assert tuple(z.shape) == lead + shape[:-1] + event
        assert z.dtype == (torch.int64 if cls is Categorical else F32) and z.device.type == cdev.type
        lp = d.log_prob(z)
        assert tuple(lp.shape) == lead + shape[:-1] and lp.dtype == F32
        if cls is Categorical:
            assert bool(((z >= 0) & (z < 5)).all())
        elif cls is OnehotCategorical:
            assert bool((z.sum(-1) == 1).all()) and bool(((z == 0) | (z == 1)).all())
        elif cls is Concrete:
            assert bool((z >= 0).all()) and float((z.sum(-1) - 1).abs().max()) < 1e-5
        else:
            assert float(torch.logsumexp(z.double(), -1).abs().max()) < 1e-5
    for g in range(len(shape)):
        dg = make(cls, lg, group_ndims=g)
        z = dg.sample(5)
        assert tuple(dg.log_prob(z).shape) == ((5,) + shape[:-1])[:len(shape) - g]
        assert tuple(dg.log_prob(z.clone()).shape) == ((5,) + shape[:-1])[:len(shape) - g]
        assert torch.allclose(dg.log_prob(z), dg.log_prob(z.clone()), rtol=1e-5, atol=1e-5)


def test_float64_and_integer_dtypes(cdev):
    lg = rand_logits((3, 4), 2, cdev, F64)
    assert Categorical(lg).sample(2).dtype == torch.int64 and Categorical(lg).log_prob(torch.zeros(3, dtype=torch.int64)).dtype == F64
    assert Categorical(lg, dtype=torch.int32).sample(2).dtype == torch.int32
    assert OnehotCategorical(lg).sample(2).dtype == F64 and Concrete(0.5, lg).sample(2).dtype == F64


def test_value_errors(cdev):
    lg = rand_logits((3, 4), 3, cdev)
    with pytest.raises(ValueError):
        Categorical(lg, group_ndims=-1)
    with pytest.raises(ValueError):
        Categorical(torch.tensor(1.0, device=cdev))
    with pytest.raises(TypeError):
        Categorical(torch.zeros(3, 4, dtype=torch.int64, device=cdev))
    with pytest.raises(TypeError):
        Categorical(lg, dtype=torch.float32)
    for tau in (0.0, -1.0, float("nan"), float("inf"), torch.tensor(-0.5)):
        with pytest.raises(ValueError):
            ExpConcrete(tau, lg)
        with pytest.raises(ValueError):
            Concrete(tau, lg)
    assert ExpConcrete(torch.tensor(0.25), lg).temperature == 0.25
    for cls in (ExpConcrete, Concrete):
        with pytest.raises(NotImplementedError):
            cls(0.5, lg, use_path_derivative=True)
    with pytest.raises(ValueError):
        OnehotCategorical(lg).log_prob(torch.zeros(3, 5, device=cdev))
    with pytest.raises(ValueError):
        Concrete(0.5, lg).log_prob(torch.full((3, 3), 1 / 3., device=cdev))
    with pytest.raises(RuntimeError):
        Categorical(lg).log_prob(None)
    with pytest.raises(TypeError):
        Categorical(lg).sample(2.5)


def test_given_values_broadcast_against_the_batch_shape(cdev):
    lg = rand_logits((3, 2, 5), 4, cdev)
    ref = td.Categorical(logits=lg.cpu().double())
    d = Categorical(lg)
    for v in (torch.tensor(2), torch.tensor([0, 4]), torch.randint(0, 5, (3, 1)), torch.randint(0, 5, (7, 3, 2)), torch.randint(0, 5, (2, 4, 1, 2))):
        lp = d.log_prob(v.to(cdev))
        want = ref.log_prob(v)
        assert tuple(lp.shape) == tuple(want.shape)
        assert float((lp.cpu().double() - want).abs().max()) < 1e-5
    oh = OnehotCategorical(lg)
    refo = td.OneHotCategorical(logits=lg.cpu().double())
    for shape in ((5,), (2, 5), (4, 3, 2, 5), (4, 1, 1, 5)):
        v = torch.nn.functional.one_hot(torch.randint(0, 5, shape[:-1]), 5).float()
        lp = oh.log_prob(v.to(cdev))
        want = refo.log_prob(v.double())
        assert tuple(lp.shape) == tuple(want.shape) and float((lp.cpu().double() - want).abs().max()) < 1e-5
    # logits that broadcast up to the value
    d1 = Categorical(rand_logits((1, 5), 5, cdev))
    v = torch.randint(0, 5, (4, 6))
    want = td.Categorical(logits=d1.logits.cpu().double()).log_prob(v)
    assert float((d1.log_prob(v.to(cdev)).cpu().double() - want).abs().max()) < 1e-5


@pytest.mark.parametrize("cls", FAMILIES)
def test_few_rows_and_many_observations_go_to_the_kernels_as_rows(cdev, cls):
    """logits [N] against a batch of 40 observations (the mixture-assignment case): the backward kernels walk the particles of a
    row in turn, so the batch is presented as 40 rows of one particle; value and gradient are those of torch.distributions."""
    N, B, tau = 6, 40, 0.7
    lg = rand_logits((N,), 120, "cpu")
    g = torch.randn(B, generator=gen(121))
    if cls is Categorical:
        v = torch.randint(0, N, (B,), generator=gen(122))
    elif cls is OnehotCategorical:
        v = torch.nn.functional.one_hot(torch.randint(0, N, (B,), generator=gen(122)), N).float()
    else:
        v = torch.log_softmax(torch.randn(B, N, generator=gen(122)), -1)
        v = v if cls is ExpConcrete else torch.exp(v)
    l64 = lg.double().requires_grad_(True)
    want = torch_log_prob(cls, l64, v.double() if v.is_floating_point() else v, tau)
    gwant, = torch.autograd.grad(want, [l64], g.double())
    l0 = lg.to(cdev).requires_grad_(True)
    with cat_host.recording() as calls:
        lp = make(cls, l0, tau=tau).log_prob(v.to(cdev))
        got, = torch.autograd.grad(lp, [l0], g.to(cdev))
    assert tuple(lp.shape) == (B,)
    assert float((lp.detach().cpu().double() - want.detach()).abs().max()) < 2e-5
    assert float((got.cpu().double() - gwant).abs().max()) < 2e-5 * (1 + float(gwant.abs().max()))
    # (name, K, the logits' shape) of a forward and a backward launch
    assert [(c.name, c.args[1], c.args[0]) for c in calls] == [(n, 1, (B, N)) for n in (calls[0].name, calls[1].name)]
    # a handful of particles over many rows stays [K, R]
    from zhusuan.distributions.categorical import fold_particles
    assert fold_particles(40, 1, 6) and not fold_particles(5, 1, 6) and not fold_particles(50, 5120, 10) and not fold_particles(50, 256, 1000)


def test_there_is_no_cpu_fallback():
    cat_host.uninstall()
    host_backend.uninstall()
    with pytest.raises(RuntimeError):
        Categorical(torch.zeros(3, 4)).sample(2)
    with pytest.raises(RuntimeError):
        Concrete(0.5, torch.zeros(3, 4)).log_prob(torch.full((3, 4), 0.25))


# ------------------------------------------------------------------------------------------------ against torch.distributions
def torch_log_prob(cls, logits, value, tau, weights=False):
    """The family's log_prob by torch.distributions, in the dtype of `logits` (CPU)."""
    if cls is Categorical:
        return td.Categorical(logits=logits).log_prob(value)
    if cls is OnehotCategorical:
        if weights:          # torch's OneHotCategorical takes the argmax of the value: general weights by its own formula
            return (value.to(logits.dtype) * torch.log_softmax(logits, -1)).sum(-1)
        return td.OneHotCategorical(logits=logits, validate_args=False).log_prob(value.to(logits.dtype))
    t = torch.tensor(tau, dtype=logits.dtype)
    if cls is ExpConcrete:
        return trc.ExpRelaxedCategorical(t, logits=logits, validate_args=False).log_prob(value.to(logits.dtype))
    return trc.RelaxedOneHotCategorical(t, logits=logits, validate_args=False).log_prob(value.to(logits.dtype))


@pytest.mark.parametrize("cls", FAMILIES)
@pytest.mark.parametrize("N", [1, 3, 10, 65])
def test_log_prob_against_torch_distributions(cdev, cls, N):
    """Within 4 x the float32-vs-float64 distance of the torch formulas themselves."""
    B, K, tau = 6, 4, 0.7
    lg = rand_logits((B, N), 10 + N, "cpu")
    if cls is Categorical:
        v = torch.randint(0, N, (K, B), generator=gen(N))
    elif cls is OnehotCategorical:
        v = torch.nn.functional.one_hot(torch.randint(0, N, (K, B), generator=gen(N)), N).float()
    else:
        y = cat_host.reference_relaxed_y(lg, rand_u((K, B, N), 20 + N), tau).float()
        v = y if cls is ExpConcrete else torch.exp(y)
        if cls is Concrete:
            v = v.clamp(min=1e-30)
    want = torch_log_prob(cls, lg.double(), v.double() if v.is_floating_point() else v, tau)
    own32 = torch_log_prob(cls, lg, v, tau).double()
    dist = float((own32 - want).abs().max())
    got = make(cls, lg.to(cdev), tau=tau).log_prob(v.to(cdev)).cpu().double()
    err = float((got - want).abs().max())
    print("%s N=%d: error %.3e, torch's own float32 distance %.3e" % (cls.__name__, N, err, dist))
    if N == 1 and cls in (Categorical, OnehotCategorical):
        assert err == 0.0
    else:
        assert err <= 4 * dist, (err, dist)


@pytest.mark.parametrize("cls", FAMILIES)
def test_gradients_against_float64_autograd(cdev, cls):
    """Gradients against float64 autograd of the torch.distributions formulas, within 16 x the float32-vs-float64 distance of
    those formulas' own gradients: the rule this suite applies to gradients (the objectives below, the HMC trajectory); the
    4 x rule is for log_prob values.  Measured on the MI355X: the largest ratio is Concrete's d log_prob / d (logits, value)
    at 4.5 x (error 4.9e-5 against torch's own 1.1e-5), every other family below 4 x."""
    B, K, N, tau = 5, 3, 7, 0.6
    lg = rand_logits((B, N), 31, "cpu")
    u = rand_u((K, B, N), 32)
    g = torch.randn(K, B, generator=gen(33))
    if cls is Categorical:
        v = torch.randint(0, N, (K, B), generator=gen(34))
    elif cls is OnehotCategorical:
        v = torch.rand(K, B, N, generator=gen(34))
    else:
        # a point well inside the simplex: d log_prob / d x of Concrete grows like 1 / x, and the largest absolute difference
        # over elements ten orders of magnitude apart (a relaxed draw at this temperature has x down to e^-30) would compare
        # the rounding of one element only
        v = torch.log_softmax(torch.randn(K, B, N, generator=gen(34)), -1)
        v = v if cls is ExpConcrete else torch.exp(v)

    def run(dtype, dev, dist_of):
        l0 = lg.to(dtype).to(dev).requires_grad_(True)
        v0 = v.to(dev) if cls is Categorical else v.to(dtype).to(dev).requires_grad_(True)
        lp = dist_of(l0, v0)
        return torch.autograd.grad(lp, [l0] + ([] if cls is Categorical else [v0]), g.to(dtype).to(dev))

    t64 = run(F64, "cpu", lambda l, x: torch_log_prob(cls, l, x, tau, weights=True))
    t32 = run(F32, "cpu", lambda l, x: torch_log_prob(cls, l, x, tau, weights=True))
    got = run(F32, cdev, lambda l, x: make(cls, l, tau=tau).log_prob(x))
    held_to_the_rule(cls.__name__, zip(("d/dlogits", "d/dvalue"), got, t32, t64))

    if cls in (ExpConcrete, Concrete):
        # the relaxed draw and its log-density: d (sum gz z + sum g lp) / d logits
        gz = torch.randn(K, B, N, generator=gen(35))

        def truth(dtype):
            l0 = lg.to(dtype).requires_grad_(True)
            y = cat_host.reference_perturbed(l0, u).to(dtype) / tau
            y = y - torch.logsumexp(y, -1, keepdim=True)
            z = y if cls is ExpConcrete else torch.exp(y)
            lp = torch_log_prob(cls, l0, z, tau)
            return torch.autograd.grad((gz.to(dtype) * z).sum() + (g.to(dtype) * lp).sum(), [l0])[0]
        l0 = lg.to(cdev).requires_grad_(True)
        d = make(cls, l0, tau=tau)
        with zs.inject_epsilon([u]):
            z = d.sample(K)
        lp = d.log_prob(z)
        got, = torch.autograd.grad((gz.to(cdev) * z).sum() + (g.to(cdev) * lp).sum(), [l0])
        held_to_the_rule(cls.__name__, [("draw", got, truth(F32), truth(F64))])
        # is_reparameterized=False: the draw is a constant, the density keeps its direct dependence on logits
        l1 = lg.to(cdev).requires_grad_(True)
        d = make(cls, l1, tau=tau, is_reparameterized=False)
        with zs.inject_epsilon([u]):
            z1 = d.sample(K)
        assert not z1.requires_grad and torch.equal(z1, z.detach())
        got1, = torch.autograd.grad((g.to(cdev) * d.log_prob(z1)).sum(), [l1])
        l2 = lg.double().requires_grad_(True)
        want1, = torch.autograd.grad((g.double() * torch_log_prob(cls, l2, z.detach().cpu().double(), tau)).sum(), [l2])
        assert float((got1.cpu().double() - want1).abs().max()) <= 1e-4 * (1 + float(want1.abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1, 3, 65])
def test_gradcheck_of_the_float64_functions(N):
    from zhusuan.distributions import _cat_functions as F
    dev = torch.device("cuda:0")
    K, R, tau = 2, 3, 0.8
    lg = rand_logits((R, N), 40 + N, dev, F64).requires_grad_(True)
    u = rand_u((K, R, N), 41 + N, F64).to(dev)
    idx = torch.randint(0, N, (K, R), generator=gen(42)).to(dev)
    x = torch.rand(K, R, N, dtype=F64, generator=gen(43)).to(dev).requires_grad_(True)
    y = cat_host.reference_relaxed_y(lg.detach().cpu(), u.cpu(), tau).to(dev).requires_grad_(True)
    kw = dict(eps=1e-6, atol=1e-6, rtol=1e-5, nondet_tol=0.0)
    assert torch.autograd.gradcheck(lambda l: F.CatSampleLogProb.apply(l, u, 0, 0, None, K, True)[2], (lg,), **kw)
    assert torch.autograd.gradcheck(lambda l: F.CatLogProb.apply(l, idx, K, False), (lg,), **kw)
    assert torch.autograd.gradcheck(lambda l, v: F.CatLogProb.apply(l, v, K, True), (lg, x), **kw)
    for e in (False, True):
        assert torch.autograd.gradcheck(lambda l: [t for t in F.RelaxedSampleLogProb.apply(l, u, 0, 0, None, K, tau, e, True) if t is not None],
                                        (lg,), **kw)
        assert torch.autograd.gradcheck(lambda l, v: F.RelaxedLogProb.apply(l, v, K, tau, e), (lg, y), **kw)


# ------------------------------------------------------------------------------------------------ launches and streams
@pytest.mark.parametrize("cls", FAMILIES)
def test_own_draw_then_log_prob_is_one_launch_each_way(cdev, cls):
    """Counted through the record of the binding's calls, on both back-ends."""
    with cat_host.recording() as calls:
        lg = rand_logits((4, 3, 6), 50, cdev).requires_grad_(True)
        d = make(cls, lg, group_ndims=1)
        z = d.sample(5)
        lp = d.log_prob(z)
        lp0 = d._log_prob_sum(None, 0)
        assert tuple(lp.shape) == (5, 4) and tuple(lp0.shape) == (5, 4, 3)
        assert len(calls) == 1 and calls[0].name in ("sample_logprob", "relaxed_sample_logprob")
        (lp.sum() + (z.sum() if z.requires_grad else 0.0)).backward()
        assert len(calls) == 2 and calls[1].name in ("logprob_bwd", "relaxed_sample_logprob_bwd")
        assert "one launch" in zs.explain(d) and zs.explain(d).startswith(("C1", "C3")) and d.last_path["why"] is None
        d.log_prob(z.detach().clone())
        assert len(calls) == 3 and calls[2].name in ("logprob", "relaxed_logprob") and zs.explain(d).startswith(("C2", "C4"))
        # an output that never entered the loss costs no backward launch and no dense zero gradient
        n = len(calls)
        d2 = make(cls, lg)
        z2 = d2.sample(3)
        if z2.requires_grad:
            (z2 * z2).sum().backward()          # the draw alone: the log-density brings no gradient
            assert len(calls) == n + 2 and calls[-1].name == "relaxed_sample_logprob_bwd"
        else:
            assert d2.log_prob(z2).sum().requires_grad and len(calls) == n + 1
    print("launches on %s: %s" % (cdev.type, [c.name for c in calls]))


@pytest.mark.parametrize("cls", FAMILIES)
def test_injected_noise_reference_stream_and_seeds_reproduce(cdev, cls):
    lg = rand_logits((4, 6), 60, cdev)
    u = rand_u((3, 4, 6), 61)
    d = make(cls, lg)
    with zs.inject_epsilon([u, u]):
        a, b = d.sample(3), d.sample(3)
    assert torch.equal(a, b)
    if cls in (Categorical, OnehotCategorical):
        want = cat_host.reference_sample(lg.cpu(), u)[0]
        assert torch.equal(a.cpu() if cls is Categorical else a.argmax(-1).cpu(), want)
    with pytest.raises(RuntimeError):
        with zs.inject_epsilon([u[0]]):
            d.sample(3)
    torch.manual_seed(7)
    with zs.reference_rng():
        a = d.sample(3)
    torch.manual_seed(7)
    ur = torch.rand(3, 4, 6)
    with zs.inject_epsilon([ur]):
        b = d.sample(3)
    assert torch.equal(a, b)
    seed_all(9)
    a1, a2 = d.sample(3), d.sample(3)
    seed_all(9)
    b1, b2 = d.sample(3), d.sample(3)
    assert torch.equal(a1, b1) and torch.equal(a2, b2) and not torch.equal(a1, a2)


@pytest.mark.gpu
@pytest.mark.parametrize("cls", [OnehotCategorical, Concrete])
def test_device_rng_reproduces_and_a_graphed_step_draws_fresh_numbers(cls):
    dev = torch.device("cuda:0")
    lg = rand_logits((16, 6), 70, dev).requires_grad_(True)
    outs = []
    for _ in range(2):
        rng = zs.DeviceRNG(dev, seed=5)
        with zs.device_rng(rng):
            rng.begin_step()
            outs.append(make(cls, lg).sample(4).detach().clone())
    assert torch.equal(outs[0], outs[1])
    rng = zs.DeviceRNG(dev, seed=11)
    held = {}

    def compute():
        rng.begin_step()
        d = make(cls, lg, tau=0.5)
        z = d.sample(4)
        loss = d.log_prob(z).sum() + (z * z).sum()
        lg.grad = None
        loss.backward()
        held['z'] = z
        return loss.detach()
    step = zs.GraphedStep(compute, rng=rng, warmup=3)
    assert step.captured, step.capture_error
    step()
    torch.cuda.synchronize()
    z1, g1 = held['z'].detach().clone(), lg.grad.clone()
    step()
    torch.cuda.synchronize()
    assert not torch.equal(z1, held['z']) and not torch.equal(g1, lg.grad)


@pytest.mark.gpu
def test_a_tensor_temperature_raises_while_a_stream_is_captured(monkeypatch):
    """The constructor asks torch whether the current stream is capturing before it reads the tensor (as Logistic's scale check
    does); the answer is forced here, so that no capture has to be broken to see the error."""
    dev = torch.device("cuda:0")
    lg = rand_logits((3, 4), 75, dev)
    tau = torch.tensor(0.5, device=dev)
    assert Concrete(tau, lg).temperature == 0.5
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    for cls in (ExpConcrete, Concrete):
        with pytest.raises(RuntimeError, match="captured"):
            cls(tau, lg)
        assert cls(0.5, lg).temperature == 0.5          # a Python number needs no read


FREQ_LOGITS = [0.0, 1.0, -1.0, 2.0, 0.5]
FREQ_SEED = 2024


def test_frequencies_of_65536_philox_draws(cdev):
    """Pearson's statistic against softmax below 18.47, the 0.999 quantile of chi^2 with 4 degrees of freedom."""
    seed_all(FREQ_SEED)
    lg = torch.tensor(FREQ_LOGITS, device=cdev)
    z = Categorical(lg).sample(65536)
    assert tuple(z.shape) == (65536,)
    counts = torch.bincount(z.cpu(), minlength=5).double()
    expect = 65536 * torch.softmax(torch.tensor(FREQ_LOGITS, dtype=F64), 0)
    stat = float(((counts - expect) ** 2 / expect).sum())
    print("Pearson statistic %.4f" % stat)
    assert stat < 18.47


# ------------------------------------------------------------------------------------------------ nodes and objectives
class Net(BayesianNet):
    def __init__(self, build):
        super().__init__()
        self.build = build

    def forward(self, observed):
        self.observe(observed)
        self.build(self)
        return self


def test_bayesian_net_factories(cdev):
    lg = rand_logits((3, 2, 5), 80, cdev)
    obs_idx = torch.randint(0, 5, (4, 3, 2)).to(cdev)
    obs_y = torch.log_softmax(rand_logits((4, 3, 2, 5), 81, cdev), -1)

    def build(net):
        net.categorical('c', lg, n_samples=4)
        net.onehot_categorical('o', lg, n_samples=4, group_ndims=1)
        net.exp_concrete('e', 0.5, lg, n_samples=4, reduce_sum_dims=[2])
        net.concrete('k', 0.5, lg, n_samples=4, reduce_mean_dims=[1], reduce_sum_dims=[2], multiplier=3.0)
        net.stochastic_node('OnehotCategorical', 's', logits=lg, n_samples=4)
    net = Net(build).to(cdev)
    net({})
    assert tuple(net.nodes['c'].tensor.shape) == (4, 3, 2) and tuple(net.nodes['o'].tensor.shape) == (4, 3, 2, 5)
    assert tuple(net.nodes['c'].log_prob().shape) == (4, 3, 2) and tuple(net.nodes['o'].log_prob().shape) == (4, 3)
    assert tuple(net.nodes['e'].log_prob().shape) == (4, 3) and tuple(net.nodes['k'].log_prob().shape) == (4,)
    assert tuple(net.nodes['s'].log_prob().shape) == (4, 3, 2)
    net({'c': obs_idx, 'e': obs_y, 'k': torch.exp(obs_y)})
    assert net.nodes['c'].tensor is obs_idx and net.nodes['e'].tensor is obs_y
    want_c = td.Categorical(logits=lg.cpu().double()).log_prob(obs_idx.cpu())
    assert float((net.nodes['c'].log_prob().cpu().double() - want_c).abs().max()) < 1e-5
    want_e = trc.ExpRelaxedCategorical(torch.tensor(0.5, dtype=F64), logits=lg.cpu().double()).log_prob(obs_y.cpu().double())
    assert float((net.nodes['e'].log_prob().cpu().double() - want_e.sum(2)).abs().max()) < 1e-4
    want_k = trc.RelaxedOneHotCategorical(torch.tensor(0.5, dtype=F64), logits=lg.cpu().double()).log_prob(torch.exp(obs_y).cpu().double())
    assert float((net.nodes['k'].log_prob().cpu().double() - 3.0 * want_k.mean(1).sum(1)).abs().max()) < 1e-3
    with pytest.raises(ValueError):
        net.categorical(3, lg)


def test_log_joint_shape(cdev):
    lg = rand_logits((3, 2, 5), 82, cdev)

    def build(net):
        net.categorical('c', lg, n_samples=4, group_ndims=1)
        net.onehot_categorical('o', lg, n_samples=4, reduce_sum_dims=[-1])
        net.exp_concrete('e', 0.5, lg, n_samples=4, group_ndims=1)
        net.concrete('k', 0.5, lg, n_samples=4, group_ndims=1)
    net = Net(build).to(cdev)
    net({})
    lj = net.log_joint()
    assert tuple(lj.shape) == (4, 3)
    parts = sum(net.nodes[n].log_prob() for n in 'coek')
    assert torch.allclose(lj, parts)
    net({'o': torch.nn.functional.one_hot(torch.randint(0, 5, (3, 2)), 5).float().to(cdev)})
    assert tuple(net.log_joint().shape) == (4, 3)


def old_reduction_plan_of(self, x, dist, g):
    """``StochasticTensor._reduction_plan_of`` as it was before ``_event_ndims`` existed."""
    from zhusuan._shapes import broadcast_shapes
    from zhusuan.framework.stochastic_tensor import _norm_dims
    full = tuple(broadcast_shapes(tuple(torch.as_tensor(x).shape), tuple(dist.batch_shape)))
    nd = len(full) - g
    mean_dims = _norm_dims(self._reduce_mean_dims, nd)
    sum_dims = _norm_dims(self._reduce_sum_dims, nd)
    extra = 0
    while nd - 1 - extra >= 0 and (nd - 1 - extra) in sum_dims and (nd - 1 - extra) not in mean_dims:
        extra += 1
    return full, nd, mean_dims, sum_dims, extra


def test_pre_existing_families_are_bit_identical_with_the_old_reduction_plan(cdev, monkeypatch):
    from zhusuan.framework.stochastic_tensor import StochasticTensor
    mean = rand_logits((3, 4, 6), 90, cdev).requires_grad_(True)
    eps = [torch.randn(5, 3, 4, 6, generator=gen(91)), rand_u((5, 3, 4, 6), 93)]
    x = (torch.rand(3, 4, 6, generator=gen(92)) < 0.5).float().to(cdev)

    def build(net):
        z = net.normal('z', mean=mean, std=torch.ones_like(mean), n_samples=5, reduce_sum_dims=[3], reduce_mean_dims=[1])
        net.bernoulli('x', logits=z, group_ndims=1, reduce_sum_dims=[2], multiplier=2.0)
        net.stochastic_node('Logistic', 'l', loc=mean, scale=torch.ones_like(mean), n_samples=5, group_ndims=2)

    def run():
        net = Net(build).to(cdev)
        seed_all(3)
        with zs.inject_epsilon(eps, strict=False):
            net({'x': x})
            lps = [net.nodes[n].log_prob() for n in ('z', 'x', 'l')]
        g, = torch.autograd.grad(lps[0].sum() + lps[1].sum() + lps[2].sum(), [mean])
        return lps + [g]
    new = run()
    monkeypatch.setattr(StochasticTensor, "_reduction_plan_of", old_reduction_plan_of)
    old = run()
    for a, b in zip(new, old):
        assert a.shape == b.shape and torch.equal(a, b)


# the three objectives over D = 2 latents of N = 4 categories, B = 3, K = 5
OB, OK_, OD, ON, OX, OTAU = 3, 5, 2, 4, 6, 0.6


def objective_setup(dev, dtype):
    g = gen(100)
    P = dict(enc=0.7 * torch.randn(OX, OD * ON, generator=g, dtype=F64), dec=0.7 * torch.randn(OD * ON, OX, generator=g, dtype=F64),
             bias=0.3 * torch.randn(OX, generator=g, dtype=F64))
    P = {k: v.to(dtype).to(dev).requires_grad_(True) for k, v in P.items()}
    x = (torch.rand(OB, OX, generator=g) < 0.5).to(dtype).to(dev)
    return P, x


def zs_objective(mode, dev, P, x, u):
    relaxed = mode == 'sgvb'
    K = OK_ if mode == 'vimco' else None

    def q(net):
        lg = (net.observed['x'] @ P['enc']).reshape(OB, OD, ON)
        if relaxed:
            net.exp_concrete('z', OTAU, lg, n_samples=K, group_ndims=1)
        else:
            net.onehot_categorical('z', lg, n_samples=K, group_ndims=1)

    def p(net):
        prior = torch.zeros(OB, OD, ON, dtype=x.dtype, device=dev)
        if relaxed:
            z = torch.exp(net.exp_concrete('z', OTAU, prior, n_samples=K, group_ndims=1))
        else:
            z = net.onehot_categorical('z', prior, n_samples=K, group_ndims=1)
        net.bernoulli('x', logits=z.reshape(tuple(z.shape[:-2]) + (OD * ON,)) @ P['dec'] + P['bias'], group_ndims=1)
    gen, var = Net(p).to(dev), Net(q).to(dev)
    obj = (ImportanceWeightedObjective(gen, var, axis=0, estimator='vimco') if mode == 'vimco'
           else ELBO(gen, var, estimator='reinforce' if mode == 'reinforce' else 'sgvb')).to(dev)
    with zs.inject_epsilon([u, u]):          # the objectives draw every latent twice and use the second draw
        loss = obj({'x': x})
    return loss, torch.autograd.grad(loss, list(P.values()), allow_unused=True)


def torch_objective(mode, dev, dtype, x, u):
    """The same model with torch.distributions on the CPU in `dtype`; the objectives' own epilogue on (log p, log q)."""
    P, _ = objective_setup("cpu", dtype)
    xc = x.detach().cpu().to(dtype)
    lg = (xc @ P['enc']).reshape(OB, OD, ON)
    K = OK_ if mode == 'vimco' else 1
    noise = -torch.log(-torch.log(u.to(dtype).reshape(K, OB, OD, ON)))
    if mode == 'sgvb':
        a = (lg[None] + noise) / OTAU
        y = a - torch.logsumexp(a, -1, keepdim=True)
        tau = torch.tensor(OTAU, dtype=dtype)
        logq = trc.ExpRelaxedCategorical(tau, logits=lg).log_prob(y).sum(-1)
        logpz = trc.ExpRelaxedCategorical(tau, logits=torch.zeros(OB, OD, ON, dtype=dtype)).log_prob(y).sum(-1)
        z = torch.exp(y)
    else:
        idx = (lg.detach()[None] + noise).argmax(-1)
        z = torch.nn.functional.one_hot(idx, ON).to(dtype)
        logq = td.OneHotCategorical(logits=lg).log_prob(z).sum(-1)
        logpz = td.OneHotCategorical(logits=torch.zeros(OB, OD, ON, dtype=dtype)).log_prob(z).sum(-1)
    logits_x = z.reshape(K, OB, OD * ON) @ P['dec'] + P['bias']
    logpx = td.Bernoulli(logits=logits_x).log_prob(xc[None].expand(K, OB, OX)).sum(-1)
    logp = logpz + logpx
    if mode != 'vimco':
        logp, logq = logp[0], logq[0]
    obj = (ImportanceWeightedObjective(Net(None), Net(None), axis=0, estimator='vimco') if mode == 'vimco'
           else ELBO(Net(None), Net(None), estimator='reinforce' if mode == 'reinforce' else 'sgvb'))
    obj = obj.to(dev)
    lp, lq = logp.to(dev), logq.to(dev)
    loss = obj.vimco(lp, lq) if mode == 'vimco' else (obj.reinforce(lp, lq) if mode == 'reinforce' else obj.sgvb(lp, lq))
    return loss, torch.autograd.grad(loss, list(P.values()), allow_unused=True)


@pytest.mark.parametrize("mode", ["vimco", "reinforce", "sgvb"])
def test_objectives_over_categorical_latents(cdev, mode):
    """Value and parameter gradients against the same model written with torch.distributions in float64 with the same injected
    u, within 16 x that model's own float32-vs-float64 distance (the HMC sampler test's rule)."""
    K = OK_ if mode == 'vimco' else 1
    u = rand_u(((K,) if K > 1 else ()) + (OB, OD, ON), 101)
    P, x = objective_setup(cdev, F32)
    loss, grads = zs_objective(mode, cdev, P, x, u)
    l64, g64 = torch_objective(mode, cdev, F64, x, u)
    l32, g32 = torch_objective(mode, cdev, F32, x, u)
    pairs = [("loss", loss, l32, l64)] + [(n, a, b, c) for n, a, b, c in zip(P.keys(), grads, g32, g64)]
    for name, a, b, c in pairs:
        assert (a is None) == (c is None), name
    held_to_the_rule(mode, [p for p in pairs if p[1] is not None])
