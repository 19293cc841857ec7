"""Every ``torch.autograd.Function`` of the package against float64 finite differences, and the float32 kernels against
their float64 twins.

1. ``GRADIENT_CHECKS`` names, for every Function subclass of ``zhusuan._ops`` and ``zhusuan.invertible._functions``, how its
   backward is held to its forward: central finite differences here, or -- for the objectives whose "gradient" is by the
   reference's design NOT the derivative of the returned value -- the existing test that pins it to the float64 restatement of
   the reference.  ``test_every_function_is_listed`` fails when a Function is added without an entry.
2. ``torch.autograd.gradcheck(eps=1e-6, atol=1e-6, rtol=1e-6, nondet_tol=0)`` in float64 on both back-ends (``host``: the C
   oracle behind the ABI; ``hip``: the kernels), through the public classes.  Central differences with h = 1e-6 on operands of
   order 1 carry a truncation error of ~1e-12 and a rounding error of ~1e-10 |f|; a wrong factor, sign, axis or missing term
   is of order 1.  Inputs are asserted to stay away from every kink (ReLU, the support of Uniform, the +1e-8 of Bernoulli).
   Each case runs with all inputs differentiated, each input alone, one output at a time, and with an incoming gradient that
   is a non-contiguous view resp. an expanded scalar (gradcheck itself only feeds contiguous one-hot gradients).
3. (gpu) value and every gradient of the float32 kernels against the float64 kernels at the shapes that reach each float32
   kernel form.  The bound is the reference arithmetic's own: 16 x the distance of the float32 C oracle (``host``) from the
   float64 truth, floored at 4 * 2^-24 * max|truth|.
"""
import contextlib
import inspect
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import host_routing
from flow_host import fdev  # noqa: F401  (fixture)
import flow_host

import zhusuan as zs
from zhusuan import _hip, _ops
from zhusuan.distributions import Normal, Bernoulli, Logistic, Uniform, FlowDistribution
from zhusuan.framework.bn import BayesianNet
from zhusuan.invertible import _functions as F
from zhusuan.invertible.base import RevNet
from zhusuan.invertible.coupling import MaskCoupling, Coupling
from zhusuan.invertible.made import MADE
from zhusuan.invertible.scaling import Scaling
from zhusuan.variational.elbo import ELBO

F64, F32 = torch.float64, torch.float32
FD, SURROGATE = "finite differences", "surrogate"

# Function -> (how it is checked, the test that holds a surrogate's gradients to the reference's own -- captured from it or
# restated in float64 --, why: the reference expression in oracle/zs_oracle.py that decides it)
GRADIENT_CHECKS = {
    "zhusuan._ops.NormalSampleLogProb": (FD, None, "z = mu + sigma eps and log N(z): reparameterised draws are differentiable in (mu, sigma)"),
    "zhusuan._ops.NormalSampleLogProbPair": (FD, None, "two such draws; float32 only, so it is checked against the float64 single draw (section 3)"),
    "zhusuan._ops.NormalLogProb": (FD, None, "a plain log-density"),
    "zhusuan._ops.BernoulliLogProb": (FD, None, "a plain log-mass, linear in the observation"),
    "zhusuan._ops.IWReduce": (SURROGATE, "test_objectives.py::test_iw_estimators_golden",
                              "oracle.iw_term: (softmax(l).detach() * l).sum(), plus VIMCO's detached learning signal"),
    "zhusuan._ops.IWObjective": (SURROGATE, "test_objectives.py::test_iw_estimators_golden",
                                 "oracle.iw_sgvb / iw_vimco: the same costs with the batch mean"),
    "zhusuan._ops.BernoulliIWObjective": (SURROGATE, "test_end_to_end.py::test_iwae",
                                          "oracle.iwae_loss: iw_sgvb / iw_vimco over the fused generator side"),
    "zhusuan._ops.ScalarObjective": (FD, None, "sum_t c_t * x_t.sum(): linear, nothing detached"),
    "zhusuan._ops.LogMeanExpRows": (FD, None, "oracle.log_mean_exp detaches nothing"),
    "zhusuan._ops.LogisticSampleLogProb": (FD, None, "z = loc + scale * logit(u) and its log-density"),
    "zhusuan._ops.LogisticLogProb": (FD, None, "a plain log-density"),
    "zhusuan._ops.UniformSample": (FD, None, "low + (high - low) u: the pathwise gradient of the reparameterised draw"),
    "zhusuan._ops.UniformLogProb": (FD, None, "-log(high - low) inside the support"),
    "zhusuan._ops.ReinforceEpilogue": (SURROGATE, "test_reinforce.py::test_product_reinforce_golden",
                                       "oracle.elbo_reinforce: -(logp + l_signal.detach() * logq), and a moving mean updated in place"),
    "zhusuan._ops.LogJointScalar": (FD, None, "oracle.elbo_sgvb over plain log-probabilities"),
    "zhusuan._ops.NormalSampleLogProbMulti": (FD, None, "NormalSampleLogProb for several nodes"),
    "zhusuan._ops.ParticleLinear": (FD, None, "a dense layer"),
    "zhusuan._ops.ParticleMLP": (FD, None, "a chain of dense layers"),
    "zhusuan._ops.DenseLayer": (FD, None, "act(x w^T + b)"),
    "zhusuan.invertible._functions.Split": (FD, None, "mask * x, or every other column"),
    "zhusuan.invertible._functions.Merge": (FD, None, "x plus the masked shift"),
    "zhusuan.invertible._functions.Scale": (FD, None, "x * exp(log_scale) and sum(log_scale)"),
    "zhusuan.invertible._functions.MadeAffine": (FD, None, "(x - m) exp(-loga) and -loga"),
    "zhusuan.invertible._functions.Tail": (FD, None, "row-summed base log-density plus the log-det (base parameters are constants)"),
}


def _functions_of(module):
    return sorted("%s.%s" % (module.__name__, n) for n, c in vars(module).items()
                  if inspect.isclass(c) and issubclass(c, torch.autograd.Function) and c.__module__ == module.__name__)


def test_every_function_is_listed():
    found = _functions_of(_ops) + _functions_of(F)
    assert len(found) >= 24
    assert sorted(GRADIENT_CHECKS) == sorted(found), set(found) ^ set(GRADIENT_CHECKS)
    here = os.path.dirname(os.path.abspath(__file__))
    for name, (how, test, why) in GRADIENT_CHECKS.items():
        assert how in (FD, SURROGATE) and why, name
        if how == FD:
            assert test is None, name
            assert name.rsplit(".", 1)[1] in COVERED_BY_FINITE_DIFFERENCES, name
        else:
            fname, tname = test.split("::")
            with open(os.path.join(here, fname)) as fh:
                assert "\ndef %s(" % tname in fh.read(), test


# the Functions the cases below reach (each test notes the ones it saw run; the last test of the file compares)
COVERED_BY_FINITE_DIFFERENCES = {
    "NormalSampleLogProb", "NormalSampleLogProbPair", "NormalLogProb", "BernoulliLogProb", "ScalarObjective", "LogMeanExpRows",
    "LogisticSampleLogProb", "LogisticLogProb", "UniformSample", "UniformLogProb", "LogJointScalar", "NormalSampleLogProbMulti",
    "ParticleLinear", "ParticleMLP", "DenseLayer", "Split", "Merge", "Scale", "MadeAffine", "Tail"}


# ---------------------------------------------------------------------------------------------------------------------
# plumbing
# ---------------------------------------------------------------------------------------------------------------------
def _t(a, dtype, dev):
    """float32 numbers, widened exactly to `dtype`: the float32 and float64 runs of section 3 see the same operands."""
    return torch.tensor(np.asarray(a, dtype=np.float32), device=dev).to(dtype)


def _tup(o):
    return tuple(o) if isinstance(o, (tuple, list)) else (o,)


def _diff(outs):
    return tuple(o for o in _tup(outs) if isinstance(o, torch.Tensor) and o.requires_grad)


def _weight_t(o, j):
    """A fixed weight tensor for output `o`, stored transposed: the view handed out has o's shape and reversed strides."""
    rs = np.random.RandomState(1000 + j)
    w = _t(0.5 + rs.uniform(size=tuple(reversed(o.shape))), o.dtype, o.device)
    return w.permute(*reversed(range(o.dim()))) if o.dim() else w


@contextlib.contextmanager
def kernel_calls():
    """Names of the C-ABI entry points called inside (a spy on the kernel library's ``call``)."""
    klib = _hip.lib()
    names, orig, own = [], klib.call, klib.__dict__.get("call")

    def spy(name, *a):
        names.append(name)
        return orig(name, *a)
    klib.call = spy
    try:
        yield names
    finally:
        if own is None:
            del klib.call
        else:
            klib.call = own


def _gradcheck(f, inputs):
    assert torch.autograd.gradcheck(f, tuple(inputs), eps=1e-6, atol=1e-6, rtol=1e-6, nondet_tol=0.0)


def fd_check(inputs, f, ran=()):
    """Section 2's protocol for one case.  `inputs`: float64 leaves; `f(*inputs)`: a tensor or a tuple of tensors.
    `ran`: entry points (without the _f64 suffix) that must have been called."""
    inputs = list(inputs)
    for t in inputs:
        assert t.dtype == F64 and t.is_leaf
    n = len(inputs)
    masks = [[True] * n] + ([[i == j for j in range(n)] for i in range(n)] if n > 1 else [])
    with kernel_calls() as names:
        for m in masks:                               # all inputs, then each alone (the needs_input_grad subsets)
            for t, on in zip(inputs, m):
                t.requires_grad_(on)
            _gradcheck(f, inputs)                     # (a tuple of outputs: one at a time, the others' gradients undefined)
        for t in inputs:
            t.requires_grad_(True)
        n_out = len(_diff(f(*inputs)))
        if n_out > 1:
            for j in range(n_out):                    # only one output returned: the other never enters a graph
                _gradcheck(lambda *a, j=j: _diff(f(*a))[j], inputs)
        # the incoming gradient is an expanded scalar
        _gradcheck(lambda *a: sum(o.sum() for o in _diff(f(*a))), inputs)
        # the incoming gradient is a non-contiguous view
        seen = []

        def strided(*a):
            total = 0
            for j, o in enumerate(_diff(f(*a))):
                if sum(d > 1 for d in o.shape) >= 2:
                    o.register_hook(lambda g: seen.append(g.is_contiguous()) if g is not None else None)
                total = total + (o * _weight_t(o, j)).sum()
            return total
        _gradcheck(strided, inputs)
        if any(sum(d > 1 for d in o.shape) >= 2 for o in _diff(f(*inputs))):
            assert seen and not all(seen), "the strided variant never delivered a non-contiguous gradient"
    for r in ran:
        assert r + "_f64" in names, (r, sorted(set(names)))
    return names


def _std_arg(kind, raw):
    """Scales are exp(0.3 n): `raw` = 0.3 n is the log-std; Normal(std=) gets its exponential."""
    return np.exp(raw) if kind == "std" else raw


# ---------------------------------------------------------------------------------------------------------------------
# 2a. log-densities of a given value: Normal(std=), Normal(logstd=), Logistic, Uniform
# ---------------------------------------------------------------------------------------------------------------------
LAYOUTS = [  # mean, scale, value, what the layout reaches
    ((2, 3), (2, 3), (4, 2, 3), "ksum"),
    ((2, 3), (), (2, 3), "scalar_period"),
    ((1, 3), (2, 1), (2, 3), "materialised"),
    ((2, 3), (3,), (5, 2, 3), "mixed_periods"),
    ((4, 2, 3), (2, 3), (2, 3), "periodic_value"),
]
_LAYOUT_IDS = [l[3] for l in LAYOUTS]


def locscale_logprob_case(family, mshape, sshape, vshape, g, dtype, dev, seed=0):
    rs = np.random.RandomState(seed)
    mean = _t(rs.standard_normal(mshape), dtype, dev)
    raw = 0.3 * rs.standard_normal(sshape)
    value = _t(rs.standard_normal(vshape), dtype, dev)
    if family in ("std", "logstd"):
        scale = _t(_std_arg(family, raw), dtype, dev)

        def f(mean, scale, value):
            return Normal(mean=mean, **{family: scale}, group_ndims=g).log_prob(value)
    else:
        scale = _t(np.exp(raw), dtype, dev)

        def f(mean, scale, value):
            return Logistic(loc=mean, scale=scale, group_ndims=g).log_prob(value)
    return [mean, scale, value], f


@pytest.mark.parametrize("g", [0, 1, 2])
@pytest.mark.parametrize("mshape,sshape,vshape,tag", LAYOUTS, ids=_LAYOUT_IDS)
@pytest.mark.parametrize("family", ["std", "logstd", "logistic"])
def test_fd_locscale_log_prob(dev, family, mshape, sshape, vshape, tag, g):
    inputs, f = locscale_logprob_case(family, mshape, sshape, vshape, g, F64, dev)
    base = "zs_logistic_logprob" if family == "logistic" else "zs_normal_logprob"
    # the K-summed backward serves parameters [R, D] repeated over the particles, the element-wise one + fold() the rest
    # (with both trailing axes folded there is no particle axis left)
    fd_check(inputs, f, ran=[base, base + ("_bwd_ksum" if (tag == "ksum" and g < 2) else "_bwd")])


def uniform_logprob_case(lshape, hshape, vshape, g, dtype, dev, seed=0):
    rs = np.random.RandomState(seed)
    low = _t(-2.0 + 0.3 * np.tanh(rs.standard_normal(lshape)), dtype, dev)
    high = _t(2.0 + 0.3 * np.tanh(rs.standard_normal(hshape)), dtype, dev)
    value = _t(1.5 * np.tanh(rs.standard_normal(vshape)), dtype, dev)
    assert float((value - low.max()).min()) >= 1e-2 and float((high.min() - value).min()) >= 1e-2       # inside the support

    def f(low, high, value):
        return Uniform(low=low, high=high, group_ndims=g).log_prob(value)
    return [low, high, value], f


@pytest.mark.parametrize("g", [0, 1, 2])
@pytest.mark.parametrize("lshape,hshape,vshape,tag", LAYOUTS, ids=_LAYOUT_IDS)
def test_fd_uniform_log_prob(dev, lshape, hshape, vshape, tag, g):
    inputs, f = uniform_logprob_case(lshape, hshape, vshape, g, F64, dev)
    fd_check(inputs, f, ran=["zs_uniform_logprob"])


BERNOULLI_LAYOUTS = [((4, 2, 5), (2, 5)), ((2, 5), (2, 5)), ((2, 5), (4, 2, 5))]       # parameter, observation


def bernoulli_case(kind, pshape, xshape, g, dtype, dev, seed=0):
    rs = np.random.RandomState(seed)
    if kind == "probs":
        par = _t(rs.uniform(0.05, 0.95, pshape), dtype, dev)
        assert 0.05 <= float(par.min()) and float(par.max()) <= 0.95
    else:
        par = _t(np.clip(1.5 * rs.standard_normal(pshape), -3, 3), dtype, dev)
        assert float(par.abs().max()) <= 3
    x = _t(rs.uniform(0, 1, xshape), dtype, dev)

    def f(par, x):
        return Bernoulli(**{kind: par}, group_ndims=g).log_prob(x)
    return [par, x], f


@pytest.mark.parametrize("g", [0, 1, 2])
@pytest.mark.parametrize("pshape,xshape", BERNOULLI_LAYOUTS, ids=["periodic_x", "same", "repeated_p"])
@pytest.mark.parametrize("kind", ["probs", "logits"])
def test_fd_bernoulli_log_prob(dev, kind, pshape, xshape, g):
    inputs, f = bernoulli_case(kind, pshape, xshape, g, F64, dev)
    fwd = "zs_bernoulli_logits_logprob" if kind == "logits" else "zs_bernoulli_logprob"
    fd_check(inputs, f, ran=[fwd, fwd + "_bwd", "zs_bernoulli_logprob_bwd_x"])


# ---------------------------------------------------------------------------------------------------------------------
# 2b. the sampling Functions: (draw, fused log-density) with the draw injected
# ---------------------------------------------------------------------------------------------------------------------
SAMPLE_LAYOUTS = [((2, 3), (2, 3), "same"), ((2, 3), (), "scalar_scale"), ((1, 3), (2, 1), "expanded")]
_SAMPLE_IDS = [l[2] for l in SAMPLE_LAYOUTS]


def normal_sample_case(kind, mshape, sshape, K, g, dtype, dev, seed=0):
    """g >= 1: ``log_prob`` of the draw IS the sampling kernel's second output; g = 0: the draw goes on into K2."""
    rs = np.random.RandomState(seed)
    mean = _t(rs.standard_normal(mshape), dtype, dev)
    scale = _t(_std_arg(kind, 0.3 * rs.standard_normal(sshape)), dtype, dev)
    eps = _t(rs.standard_normal(((K,) if K > 1 else ()) + tuple(mshape)), dtype, dev)

    def f(mean, scale):
        d = Normal(mean=mean, **{kind: scale}, group_ndims=g)
        z = d.sample(K, epsilon=eps)
        lp = d.log_prob(z)
        assert (lp is d._fused[1]) == (g >= 1)
        return z, lp
    return [mean, scale], f


@pytest.mark.parametrize("g", [0, 1, 2])
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("mshape,sshape,tag", SAMPLE_LAYOUTS, ids=_SAMPLE_IDS)
@pytest.mark.parametrize("kind", ["std", "logstd"])
def test_fd_normal_sample_and_its_log_density(dev, kind, mshape, sshape, tag, K, g):
    inputs, f = normal_sample_case(kind, mshape, sshape, K, g, F64, dev)
    fd_check(inputs, f, ran=["zs_normal_sample_logprob", "zs_normal_sample_logprob_bwd"])


def test_fd_normal_sample_through_inject_epsilon(dev):
    rs = np.random.RandomState(5)
    mean, std = _t(rs.standard_normal((3, 2)), F64, dev), _t(np.exp(0.3 * rs.standard_normal((3, 2))), F64, dev)
    eps = rs.standard_normal((4, 3, 2))

    def f(mean, std):
        d = Normal(mean=mean, std=std, group_ndims=1)
        with zs.inject_epsilon([eps]):
            z = d.sample(4)
        return z, d.log_prob(z)
    fd_check([mean, std], f, ran=["zs_normal_sample_logprob_bwd"])


def test_draw_that_is_not_reparameterised_has_the_log_density_gradient_of_its_value(dev):
    """``torch.normal(mean, std)`` has a zero derivative by definition, so this path is no finite-difference case: its fused
    log-density must carry exactly the gradient of ``log_prob(z.detach())`` (which section 2a ties to finite differences),
    and the draw none."""
    rs = np.random.RandomState(6)
    for K in (1, 4):
        for kind in ("std", "logstd"):
            mean = _t(rs.standard_normal((2, 3)), F64, dev).requires_grad_(True)
            scale = _t(_std_arg(kind, 0.3 * rs.standard_normal((2, 3))), F64, dev).requires_grad_(True)
            eps = _t(rs.standard_normal(((K,) if K > 1 else ()) + (2, 3)), F64, dev)
            d = Normal(mean=mean, **{kind: scale}, group_ndims=1, is_reparameterized=False)
            z = d.sample(K, epsilon=eps)
            lp = d.log_prob(z)
            assert lp is d._fused[1]
            w = _weight_t(lp, 0)
            got = torch.autograd.grad((lp * w).sum() + (z * z).sum(), [mean, scale], retain_graph=True)
            ref = Normal(mean=mean, **{kind: scale}, group_ndims=1).log_prob(z.detach())
            want = torch.autograd.grad((ref * w).sum(), [mean, scale])
            for a, b in zip(got, want):
                assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))
            gz = torch.autograd.grad(z.sum(), [mean, scale], allow_unused=True)
            assert all(v is None or not bool(v.any()) for v in gz)


def logistic_sample_case(lshape, sshape, K, g, dtype, dev, seed=0):
    rs = np.random.RandomState(seed)
    loc = _t(rs.standard_normal(lshape), dtype, dev)
    scale = _t(np.exp(0.3 * rs.standard_normal(sshape)), dtype, dev)
    u = _t(rs.uniform(0.05, 0.95, ((K,) if K > 1 else ()) + tuple(lshape)), dtype, dev)

    def f(loc, scale):
        d = Logistic(loc=loc, scale=scale, group_ndims=g)
        z = d.sample(K, uniform=u)
        return z, d.log_prob(z)
    return [loc, scale], f


@pytest.mark.parametrize("g", [0, 1, 2])
@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("lshape,sshape,tag", SAMPLE_LAYOUTS, ids=_SAMPLE_IDS)
def test_fd_logistic_sample_and_its_log_density(dev, lshape, sshape, tag, K, g):
    inputs, f = logistic_sample_case(lshape, sshape, K, g, F64, dev)
    fd_check(inputs, f, ran=["zs_logistic_sample_logprob", "zs_logistic_sample_logprob_bwd"])


def uniform_sample_case(lshape, hshape, K, dtype, dev, seed=0):
    rs = np.random.RandomState(seed)
    low = _t(-1.0 + 0.3 * np.tanh(rs.standard_normal(lshape)), dtype, dev)
    high = _t(1.0 + 0.3 * np.tanh(rs.standard_normal(hshape)), dtype, dev)
    u = _t(rs.uniform(0.05, 0.95, ((K,) if K > 1 else ()) + tuple(lshape)), dtype, dev)

    def f(low, high):
        return Uniform(low=low, high=high).sample(K, uniform=u)
    return [low, high], f


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("lshape,hshape,tag", SAMPLE_LAYOUTS + [((3,), (2, 3), "repeated_low")],
                         ids=_SAMPLE_IDS + ["repeated_low"])
def test_fd_uniform_sample_pathwise(dev, lshape, hshape, tag, K):
    inputs, f = uniform_sample_case(lshape, hshape, K, F64, dev)
    fd_check(inputs, f, ran=["zs_uniform_sample"])


MULTI_NODES = {  # per node: (shape of mu, K, n_fold, is_logstd)
    "two": [((3, 2), 4, 1, False), ((5,), 1, 1, True)],
    "three": [((2, 3), 1, 2, True), ((4,), 3, 1, False), ((2, 2, 2), 2, 1, False)],
}


def multi_sample_case(nodes, dtype, dev, seed=0):
    rs = np.random.RandomState(seed)
    meta, params, epss = [], [], []
    for shape, K, n_fold, ls in nodes:
        params += [_t(rs.standard_normal(shape), dtype, dev), _t(_std_arg("logstd" if ls else "std", 0.3 * rs.standard_normal(shape)), dtype, dev)]
        epss.append(_t(rs.standard_normal(((K,) if K > 1 else ()) + shape), dtype, dev))
        meta.append((K, K > 1, n_fold, ls, 0))

    def f(*p):
        tensors = []
        for i, e in enumerate(epss):
            tensors += [p[2 * i], p[2 * i + 1], e]
        return _ops.NormalSampleLogProbMulti.apply(tuple(meta), 0, None, *tensors)
    return params, f


@pytest.mark.parametrize("which", sorted(MULTI_NODES))
def test_fd_normal_sample_multi(dev, which):
    """(z_i, lp_i) of every node and the second handle ``alias_i`` on every draw."""
    inputs, f = multi_sample_case(MULTI_NODES[which], F64, dev)
    assert len(_diff(f(*[t.requires_grad_(True) for t in inputs]))) == 3 * len(MULTI_NODES[which])
    fd_check(inputs, f, ran=["zs_normal_sample_logprob_multi", "zs_normal_sample_logprob_multi_bwd"])


# ---------------------------------------------------------------------------------------------------------------------
# 2c. log_mean_exp, the scalar objectives
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,dim,keep", [((3, 4, 5), 0, False), ((3, 4, 5), 1, True), ((3, 4, 5), 2, False), ((3, 4, 5), (0, 2), False),
                                            ((3, 4), None, False), ((2, 70), 1, False), ((1, 1), 1, False)],
                         ids=["dim0", "dim1_keep", "dim2", "dims02", "all", "K70", "one"])
def test_fd_log_mean_exp(dev, shape, dim, keep):
    x = _t(np.random.RandomState(7).standard_normal(shape), F64, dev)
    fd_check([x], lambda x: zs.log_mean_exp(x, dim, keep), ran=["zs_log_mean_exp"])


def test_fd_scalar_objective(dev):
    rs = np.random.RandomState(8)
    shapes = [(3, 4), (), (5,), (2, 3, 2), (4, 2), (6,)]
    xs = [_t(rs.standard_normal(s), F64, dev) for s in shapes]
    coefs = [1.0, -0.5, 2.0, 0.25, -1.5, 3.0]

    def views(ts):          # a dense transposed operand, a strided one that has to be copied
        ts = list(ts)
        ts[0] = ts[0].t()
        if len(ts) > 4:
            ts[4] = ts[4][::2]
        return ts
    for n in (1, 3, 6):
        fd_check(xs[:n], lambda *a, n=n: _ops.ScalarObjective.apply(tuple(coefs[:n]), *views(a)), ran=["zs_scalar_objective"])


class _Gen(BayesianNet):
    def __init__(self, B, x_dim, z_dims, hidden):
        super().__init__()
        self.net = nn.Sequential(nn.Linear(sum(z_dims), hidden), nn.Tanh(), nn.Linear(hidden, x_dim), nn.Sigmoid())
        for i, zd in enumerate(z_dims):
            self.register_buffer("m%d" % i, torch.zeros(B, zd))
            self.register_buffer("s%d" % i, torch.ones(B, zd))
        self.n = len(z_dims)

    def forward(self, observed):
        self.observe(observed)
        zs_ = [self.normal("z%d" % i, mean=getattr(self, "m%d" % i), std=getattr(self, "s%d" % i), reduce_mean_dims=[0], reduce_sum_dims=[1])
               for i in range(self.n)]
        probs = self.net(torch.cat(zs_, 1))
        self.cache["probs"] = probs
        self.bernoulli("x", probs=probs, reduce_mean_dims=[0], reduce_sum_dims=[1])
        return self


class _Var(BayesianNet):
    def __init__(self, x_dim, z_dims, hidden):
        super().__init__()
        self.body = nn.Sequential(nn.Linear(x_dim, hidden), nn.Tanh())
        self.mean = nn.ModuleList(nn.Linear(hidden, zd) for zd in z_dims)
        self.logstd = nn.ModuleList(nn.Linear(hidden, zd) for zd in z_dims)

    def forward(self, observed):
        self.observe(observed)
        h = self.body(self.observed["x"])
        for i, (m, s) in enumerate(zip(self.mean, self.logstd)):
            self.normal("z%d" % i, mean=m(h), std=torch.exp(s(h)), reduce_mean_dims=[0], reduce_sum_dims=[1])
        return self


@pytest.mark.parametrize("z_dims", [(2,), (2, 3)], ids=["one_latent", "two_latents"])
def test_fd_logjoint_scalar_through_elbo(dev, z_dims):
    """LJ1 (and, with two latents, the multi-node sampler in front of it) inside ``ELBO`` on a net whose every parameter,
    prior and observation is float64; B = 3, x = 6, hidden = 5, Tanh instead of ReLU."""
    B, X, H = 3, 6, 5
    torch.manual_seed(0)
    model = ELBO(_Gen(B, X, z_dims, H), _Var(X, z_dims, H)).double().to(dev)
    rs = np.random.RandomState(9)
    x = _t(rs.uniform(size=(B, X)) < 0.5, F64, dev)
    eps = [rs.standard_normal((B, zd)) for zd in z_dims] * 2          # every latent is drawn twice, the second draw is used
    params = list(model.parameters())
    assert all(p.dtype == F64 for p in params) and all(b.dtype == F64 for b in model.buffers())

    def f(*_):
        with zs.inject_epsilon(eps):
            return model({"x": x})
    with kernel_calls() as names:
        f()
    said = zs.explain(model)
    assert "differ in dtype" not in said and said.startswith("LJ1"), said
    probs = model.generator.cache["probs"].detach()
    assert 0.05 <= float(probs.min()) and float(probs.max()) <= 0.95
    assert "zs_logjoint_scalar_f64" in names
    assert ("zs_normal_sample_logprob_multi_f64" in names) == (len(z_dims) > 1)
    names = fd_check(params, f, ran=["zs_logjoint_scalar", "zs_logjoint_scalar_bwd"])
    assert not any(n.endswith("_f32") for n in names)


# ---------------------------------------------------------------------------------------------------------------------
# 2d. layers
# ---------------------------------------------------------------------------------------------------------------------
def _pl_reference(h, w, relu):
    K, n_out, n_in1 = w.shape
    if h.dim() == 2:
        h = h.unsqueeze(0).expand(K, *h.shape)
    pre = (torch.bmm(h, w[:, :, :n_in1 - 1].transpose(1, 2)) + w[:, :, n_in1 - 1].unsqueeze(1)) / float(n_in1) ** 0.5
    return pre, (torch.relu(pre) if relu else pre)


MARGIN_FD = 1e-2          # finite differences move an operand by 1e-6: no pre-activation may come near its kink
MARGIN_F32 = 1e-5         # section 3: float32 and float64 must take the same branch (float32 rounds order-1 values by ~1e-7)


def particle_case(K, sizes, shared, B, dtype, dev, relu_last=False, margin=MARGIN_FD):
    """Weights and inputs of a particle MLP whose ReLU pre-activations all keep `margin` away from zero (the first seed for
    which they do; judged in float64)."""
    for seed in range(200):
        rs = np.random.RandomState(seed)
        x = _t(rs.standard_normal(((B, sizes[0]) if shared else (K, B, sizes[0]))), dtype, dev)
        ws = [_t(rs.standard_normal((K, sizes[l + 1], sizes[l] + 1)), dtype, dev) for l in range(len(sizes) - 1)]
        h, ok = x.double(), True
        for l, w in enumerate(ws):
            relu = l < len(ws) - 1 or relu_last
            pre, h = _pl_reference(h, w.double(), relu)
            ok = ok and (not relu or float(pre.abs().min()) >= margin)
        if ok:
            return x, ws
    raise AssertionError("no seed keeps the pre-activations away from zero")


@pytest.mark.parametrize("shared", [True, False], ids=["shared_h", "h_per_particle"])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("n_in,n_out", [(3, 2), (5, 4)])
@pytest.mark.parametrize("K", [1, 3])
def test_fd_particle_linear(dev, K, n_in, n_out, relu, shared):
    x, (w,) = particle_case(K, [n_in, n_out], shared, 3, F64, dev, relu_last=relu)
    fd_check([x, w], lambda h, w: zs.particle_linear(h, w, relu=relu), ran=["zs_particle_linear", "zs_particle_linear_bwd"])


@pytest.mark.parametrize("shared", [True, False], ids=["shared_x", "x_per_particle"])
@pytest.mark.parametrize("sizes", [[5, 4, 2], [5, 4, 3, 2]], ids=["two_layers", "three_layers"])
@pytest.mark.parametrize("K", [1, 3])
def test_fd_particle_mlp(dev, K, sizes, shared):
    x, ws = particle_case(K, sizes, shared, 3, F64, dev)
    fd_check([x] + ws, lambda x, *ws: zs.particle_mlp(x, ws), ran=["zs_particle_mlp", "zs_particle_mlp_bwd"])


def dense_case(act, xshape, n_out, dtype, dev, margin=MARGIN_FD):
    """(the layer is initialised in float32 and widened: the same numbers in either precision)"""
    for seed in range(200):
        torch.manual_seed(seed)
        lin = zs.Linear(xshape[-1], n_out, activation=act).to(dtype).to(dev)
        x = _t(np.random.RandomState(seed).standard_normal(xshape), dtype, dev)
        with torch.no_grad():
            pre = torch.nn.functional.linear(x.double(), lin.weight.double(), lin.bias.double())
        if act != "relu" or float(pre.abs().min()) >= margin:
            return lin, x
    raise AssertionError("no seed keeps the pre-activations away from zero")


@pytest.mark.parametrize("xshape", [(4, 3), (2, 3, 3), (1, 5)], ids=["2d", "3d", "one_row"])
@pytest.mark.parametrize("act", [None, "relu", "sigmoid"])
def test_fd_dense_layer(dev, act, xshape):
    lin, x = dense_case(act, xshape, 4, F64, dev)
    ran = ["zs_dense_act_bwd"] if act else ["zs_column_sum"]
    fd_check([x, lin.weight, lin.bias], lambda *_: lin(x), ran=ran)


def test_fd_dense_layers_in_sequential(dev):
    """``zhusuan.Sequential`` folds Linear + ReLU / Sigmoid pairs into one DenseLayer each."""
    for seed in range(200):
        torch.manual_seed(seed)
        net = zs.Sequential(zs.Linear(3, 5), nn.ReLU(), zs.Linear(5, 4), nn.Sigmoid(), zs.Linear(4, 2, bias=False)).double().to(dev)
        x = _t(np.random.RandomState(seed).standard_normal((4, 3)), F64, dev)
        with torch.no_grad():
            if float(net[0](x, activation=None).abs().min()) >= 1e-2:
                break
    else:
        raise AssertionError("no seed keeps the pre-activations away from zero")
    names = fd_check([x] + list(net.parameters()), lambda *_: net(x), ran=["zs_dense_act_bwd"])
    assert names.count("zs_dense_act_bwd_f64") >= 2


# ---------------------------------------------------------------------------------------------------------------------
# 2e. flows
# ---------------------------------------------------------------------------------------------------------------------
def _tanh_net(n_in, mid, n_out):
    return nn.Sequential(nn.Linear(n_in, mid), nn.Tanh(), nn.Linear(mid, n_out))


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("D", [2, 5])
@pytest.mark.parametrize("B", [1, 3])
def test_fd_mask_coupling(fdev, B, D, reverse):
    """Split and Merge in MASK mode, with a mask that is not 0 / 1 (a binary mask hides a swapped mask / 1 - mask)."""
    torch.manual_seed(1)
    rs = np.random.RandomState(10 * B + D)
    mask = _t(rs.uniform(0.2, 0.8, D), F64, fdev)
    layer = MaskCoupling(mask=mask, inner_nn=_tanh_net(D, 4, D)).double().to(fdev)
    x = _t(rs.standard_normal((B, D)), F64, fdev)
    with flow_host.count_launches() as c:
        fd_check([x] + list(layer.parameters()), lambda x, *_: layer(x, reverse=reverse)[0])
    assert c["split"] and c["split_bwd"] and c["merge"] and c["merge_bwd"]


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("mask_config", [0, 1])
@pytest.mark.parametrize("D", [2, 6])
@pytest.mark.parametrize("B", [1, 3])
def test_fd_coupling(fdev, B, D, mask_config, reverse):
    """Split and Merge in INTERLEAVE mode through ``Coupling`` (its inner network has a ReLU: kept away from zero)."""
    for seed in range(200):
        torch.manual_seed(seed)
        layer = Coupling(D, 4, 1, mask_config).double().to(fdev)
        x = _t(np.random.RandomState(seed).standard_normal((B, D)), F64, fdev)
        with torch.no_grad():
            pre = layer.in_block[0](x[:, (1 if mask_config else 0)::2])
        if float(pre.abs().min()) >= 1e-2:
            break
    else:
        raise AssertionError("no seed keeps the pre-activations away from zero")
    with flow_host.count_launches() as c:
        fd_check([x] + list(layer.parameters()), lambda x, *_: layer(x, reverse=reverse)[0])
    assert c["split"] and c["split_bwd"] and c["merge"] and c["merge_bwd"]


@pytest.mark.parametrize("reverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("D", [2, 5])
@pytest.mark.parametrize("B", [1, 3])
def test_fd_scaling(fdev, B, D, reverse):
    """(y, log-det); the layer works in place, so it is handed a copy of the leaf."""
    rs = np.random.RandomState(20 * B + D)
    layer = Scaling(D).double().to(fdev)
    with torch.no_grad():
        layer.log_scale.copy_(_t(0.3 * rs.standard_normal((1, D)), F64, fdev))
    x = _t(rs.standard_normal((B, D)), F64, fdev)
    with flow_host.count_launches() as c:
        fd_check([x, layer.log_scale], lambda x, _: layer(x.clone(), reverse=reverse))
    assert c["scale_fwd"] and c["scale_bwd"]


@pytest.mark.parametrize("D", [2, 5])
@pytest.mark.parametrize("B", [1, 3])
def test_fd_made_affine(fdev, B, D):
    """(u, log-det [B, D]) of MADE's forward; tanh inside the masked network."""
    torch.manual_seed(2)
    layer = MADE(D, 4, 1, activation="tanh").double().to(fdev)
    x = _t(np.random.RandomState(30 * B + D).standard_normal((B, D)), F64, fdev)
    with flow_host.count_launches() as c:
        fd_check([x] + list(layer.parameters()), lambda x, *_: layer(x))
    assert c["made_fwd"] and c["made_bwd"]


class _Probe(RevNet):
    """z = a * x + b with a log-det of the kind asked for, in plain torch: what reaches ``Tail`` is differentiable in all of
    (x, a, c), through z and through the log-det."""

    def __init__(self, a, c, kind):
        super().__init__()
        self.a, self.c, self.kind = a, c, kind

    def _forward(self, x, **kw):
        z = x * self.a + 0.1
        if self.kind == "none":
            return z, None
        if self.kind == "scalar":
            return z, (self.c * self.c).sum()
        if self.kind == "scalar1":
            return z, (self.c * self.c).sum().reshape(1)
        return z, (x * self.c).sum(1)


@pytest.mark.parametrize("kind", ["none", "scalar", "scalar1", "rows"])
@pytest.mark.parametrize("param_rows", [False, True], ids=["params_D", "params_BD"])
@pytest.mark.parametrize("base", ["normal", "logistic"])
@pytest.mark.parametrize("B,D", [(1, 2), (3, 5), (3, 2), (1, 5)])
def test_fd_flow_distribution_tail(fdev, B, D, base, param_rows, kind):
    rs = np.random.RandomState(40 * B + D)
    pshape = (B, D) if param_rows else (D,)
    loc, scale = _t(rs.standard_normal(pshape), F64, fdev), _t(np.exp(0.3 * rs.standard_normal(pshape)), F64, fdev)
    x, a, c = (_t(rs.standard_normal(s), F64, fdev) for s in ((B, D), (D,), (D,)))
    lat = Normal(mean=loc, std=scale) if base == "normal" else Logistic(loc=loc, scale=scale)

    def f(x, a, c):
        d = FlowDistribution(lat, _Probe(a, c, kind), dtype=F64)
        out = d.log_prob(x)
        assert d.last_path["path"].startswith("F-tail"), d.last_path
        return out
    with flow_host.count_launches() as cnt:
        fd_check([x, a, c], f)
    assert cnt["tail"] and cnt["tail_bwd"]


# ---------------------------------------------------------------------------------------------------------------------
# 3. the float32 kernels against their float64 twins (gpu); the bound is the float32 C oracle's own distance
# ---------------------------------------------------------------------------------------------------------------------
RATIOS = {}          # Function -> the largest |hip32 - truth| / max(|host32 - truth|, floor / 16) seen (printed by the last test)


def _evaluate(make, dtype, dev):
    """Outputs and weighted-sum gradients of a case as float64 host tensors, plus the entry points that ran."""
    inputs, f = make(dtype, dev)
    for t in inputs:
        t.requires_grad_(True)
    with kernel_calls() as names:
        outs = _diff(f(*inputs))
        loss = sum((o * _weight_t(o, j)).sum() for j, o in enumerate(outs))
        grads = torch.autograd.grad(loss, inputs, allow_unused=True)
    res = [o.detach().double().cpu() for o in outs]
    res += [torch.zeros(t.shape, dtype=F64) if g is None else g.detach().double().cpu() for t, g in zip(inputs, grads)]
    return res, names


def _on_host(make, dtype):
    with host_routing.host(flow_host.router) as dev:
        return _evaluate(make, dtype, dev)


def twin_check(function, make, ran32=()):
    dev = torch.device("cuda:0")
    truth, _ = _evaluate(make, F64, dev)
    got, names = _evaluate(make, F32, dev)
    ref, _ = _on_host(make, F32)
    for r in ran32:
        assert r + "_f32" in names, (r, sorted(set(names)))
    lines, bad = [], []
    for i, (t, g, r) in enumerate(zip(truth, got, ref)):
        assert t.shape == g.shape == r.shape
        if t.numel() == 0:
            continue
        ref_err = float((r - t).abs().max())
        floor = 4 * 2.0 ** -24 * float(t.abs().max())
        bound = max(16 * ref_err, floor)
        err = float((g - t).abs().max())
        ratio = err / (bound / 16) if bound > 0 else (0.0 if err == 0 else float("inf"))
        RATIOS[function] = max(RATIOS.get(function, 0.0), ratio)
        lines.append("tensor %d: hip32 err %.3e  host32 err %.3e  floor %.3e  ratio %.2f" % (i, err, ref_err, floor, ratio))
        if not err <= bound:
            bad.append(lines[-1])
    print("%s\n  %s" % (function, "\n  ".join(lines)))
    assert not bad, bad


# (K, R, D) members of test_cabi's NORMAL_SHAPES / BERN_SHAPES / PAIR_SHAPES and test_locscale's SHAPES: the smallest one of each
# kernel form (scalar rows, rows below / at / above a wavefront, unaligned rows, long rows, many particles)
KRD_NORMAL = [(1, 1, 1), (3, 5, 4), (3, 9, 7), (4, 1, 51), (5, 6, 40), (64, 3, 12), (2, 2, 260), (2, 3, 700)]
KRD_BERNOULLI = [(3, 4, 16), (2, 3, 783), (7, 2, 100), (1, 5, 784)]
KRD_LOCSCALE = [(1, 1, 1), (1, 7, 1), (3, 5, 4), (4, 1, 51), (64, 3, 12), (2, 2, 260), (2, 3, 700)]
KRD_PAIR = [(5, 8, 40), (7, 33, 12), (2, 1, 784)]


def _krd_id(s):
    return "K%d_R%d_D%d" % s


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["ksum", "elementwise"])
@pytest.mark.parametrize("family", ["std", "logstd"])
@pytest.mark.parametrize("krd", KRD_NORMAL, ids=_krd_id)
def test_f32_normal_log_prob_against_f64(krd, family, layout):
    K, R, D = krd
    sshape = (R, D) if layout == "ksum" else (D,)
    ksum = K > 1 and (layout == "ksum" or R == 1)          # (a [D] scale against one row IS the repeated [R, D] layout)
    ran = ["zs_normal_logprob", "zs_normal_logprob_bwd_ksum" if ksum else "zs_normal_logprob_bwd"]
    twin_check("NormalLogProb", lambda dt, dev: locscale_logprob_case(family, (R, D), sshape, (K, R, D), 1, dt, dev, seed=K + R + D), ran)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["ksum", "elementwise"])
@pytest.mark.parametrize("krd", KRD_LOCSCALE, ids=_krd_id)
def test_f32_logistic_log_prob_against_f64(krd, layout):
    K, R, D = krd
    sshape = (R, D) if layout == "ksum" else (D,)
    ksum = K > 1 and (layout == "ksum" or R == 1)
    ran = ["zs_logistic_logprob", "zs_logistic_logprob_bwd_ksum" if ksum else "zs_logistic_logprob_bwd"]
    twin_check("LogisticLogProb", lambda dt, dev: locscale_logprob_case("logistic", (R, D), sshape, (K, R, D), 1, dt, dev, seed=K + R + D), ran)


@pytest.mark.gpu
@pytest.mark.parametrize("krd", KRD_LOCSCALE, ids=_krd_id)
def test_f32_uniform_against_f64(krd):
    K, R, D = krd
    twin_check("UniformLogProb", lambda dt, dev: uniform_logprob_case((R, D), (D,), (K, R, D), 1, dt, dev, seed=K + R + D), ["zs_uniform_logprob"])
    twin_check("UniformSample", lambda dt, dev: uniform_sample_case((R, D), (D,), K, dt, dev, seed=K + R + D), ["zs_uniform_sample"])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["probs", "logits"])
@pytest.mark.parametrize("krd", KRD_BERNOULLI, ids=_krd_id)
def test_f32_bernoulli_log_prob_against_f64(krd, kind):
    K, R, D = krd
    fwd = "zs_bernoulli_logits_logprob" if kind == "logits" else "zs_bernoulli_logprob"
    twin_check("BernoulliLogProb", lambda dt, dev: bernoulli_case(kind, (K, R, D), (R, D), 1, dt, dev, seed=K + R + D),
               [fwd, fwd + "_bwd", "zs_bernoulli_logprob_bwd_x"])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["std", "logstd"])
@pytest.mark.parametrize("krd", KRD_NORMAL, ids=_krd_id)
def test_f32_normal_sample_against_f64(krd, kind):
    K, R, D = krd
    twin_check("NormalSampleLogProb", lambda dt, dev: normal_sample_case(kind, (R, D), (R, D), K, 1, dt, dev, seed=K + R + D),
               ["zs_normal_sample_logprob", "zs_normal_sample_logprob_bwd"])


@pytest.mark.gpu
@pytest.mark.parametrize("krd", KRD_LOCSCALE, ids=_krd_id)
def test_f32_logistic_sample_against_f64(krd):
    K, R, D = krd
    twin_check("LogisticSampleLogProb", lambda dt, dev: logistic_sample_case((R, D), (R, D), K, 1, dt, dev, seed=K + R + D),
               ["zs_logistic_sample_logprob", "zs_logistic_sample_logprob_bwd"])


@pytest.mark.gpu
@pytest.mark.parametrize("krd", KRD_PAIR, ids=_krd_id)
def test_f32_normal_sample_pair_against_f64(krd):
    """The pair draws in the kernel (no epsilon operand), so its draws are read back: ``philox_normal`` returns the epsilons
    of a (seed, call id), and the float64 truth and the float32 oracle are the single-draw Function on exactly those."""
    K, R, D = krd
    dev = torch.device("cuda:0")
    seed, call = 1234, 7
    rs = np.random.RandomState(K + R + D)
    mu32, sd32 = rs.standard_normal((R, D)), np.exp(0.3 * rs.standard_normal((R, D)))
    lead = (K,) if K > 1 else ()
    eps = [_ops.philox_normal(lead + (R, D), dev, seed, call + j, None, F32).cpu().numpy() for j in range(2)]

    def pair(dtype, dev_):
        mu, sd = _t(mu32, dtype, dev_), _t(sd32, dtype, dev_)
        if dtype == F32 and dev_.type == "cuda":
            return [mu, sd], lambda mu, sd: _ops.NormalSampleLogProbPair.apply(mu, sd, seed, call, None, K, K > 1, 1, True, False)

        def two(mu, sd):
            out = ()
            for e in eps:
                out += tuple(_ops.NormalSampleLogProb.apply(mu, sd, _t(e, dtype, dev_), 0, 0, None, K, K > 1, 1, True, True, False))
            return out
        return [mu, sd], two
    twin_check("NormalSampleLogProbPair", pair, ["zs_normal_sample_logprob_pair", "zs_normal_sample_logprob_bwd"])
    with kernel_calls():
        got = _ops.NormalSampleLogProbPair.apply(_t(mu32, F32, dev), _t(sd32, F32, dev), seed, call, None, K, K > 1, 1, True, False)
    for j in range(2):          # the draws read back are the pair's own
        want = _t(mu32, F32, dev) + _t(sd32, F32, dev) * _t(eps[j], F32, dev)
        assert float((got[2 * j] - want).abs().max()) <= 2 ** -22 * float(want.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("which", sorted(MULTI_NODES))
def test_f32_normal_sample_multi_against_f64(which):
    nodes = MULTI_NODES[which] + [((33, 40), 5, 1, False)]
    twin_check("NormalSampleLogProbMulti", lambda dt, dev: multi_sample_case(nodes, dt, dev),
               ["zs_normal_sample_logprob_multi", "zs_normal_sample_logprob_multi_bwd"])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 4), (5, 64), (3, 65), (2, 700)], ids=lambda s: "B%d_K%d" % s)
def test_f32_log_mean_exp_and_scalar_objective_against_f64(shape):
    def lme(dt, dev):
        x = _t(2.0 * np.random.RandomState(sum(shape)).standard_normal(shape), dt, dev)
        return [x], lambda x: zs.log_mean_exp(x, 1)

    def scalar(dt, dev):
        rs = np.random.RandomState(sum(shape))
        xs = [_t(rs.standard_normal(s), dt, dev) for s in (shape, (), (shape[1],))]
        return xs, lambda *a: _ops.ScalarObjective.apply((1.0, -0.5, 2.0), a[0].t(), a[1], a[2])
    twin_check("LogMeanExpRows", lme, ["zs_log_mean_exp"])
    twin_check("ScalarObjective", scalar, ["zs_scalar_objective"])


@pytest.mark.gpu
@pytest.mark.parametrize("K,sizes,B", [(1, [3, 2], 3), (3, [5, 4], 3), (10, [8, 50], 70), (4, [50, 1], 33)],
                         ids=["K1_3x2", "K3_5x4", "K10_8x50_B70", "K4_50x1_B33"])
def test_f32_particle_linear_against_f64(K, sizes, B):
    for shared in (True, False):
        for relu in (False, True):
            def make(dt, dev):
                x, (w,) = particle_case(K, sizes, shared, B, dt, dev, relu_last=relu, margin=MARGIN_F32)
                return [x, w], lambda h, w: zs.particle_linear(h, w, relu=relu)
            twin_check("ParticleLinear", make, ["zs_particle_linear", "zs_particle_linear_bwd"])


@pytest.mark.gpu
@pytest.mark.parametrize("K,sizes,B", [(1, [5, 4, 2], 3), (3, [5, 4, 3, 2], 3), (10, [8, 50, 1], 70)], ids=["two", "three", "bnn_shaped"])
def test_f32_particle_mlp_against_f64(K, sizes, B):
    for shared in (True, False):
        def make(dt, dev):
            x, ws = particle_case(K, sizes, shared, B, dt, dev, margin=MARGIN_F32)
            return [x] + ws, lambda x, *ws: zs.particle_mlp(x, ws)
        twin_check("ParticleMLP", make, ["zs_particle_mlp", "zs_particle_mlp_bwd"])


@pytest.mark.gpu
@pytest.mark.parametrize("act", [None, "relu", "sigmoid"])
@pytest.mark.parametrize("xshape,n_out", [((4, 3), 4), ((70, 40), 65)], ids=["small", "two_tiles"])
def test_f32_dense_layer_against_f64(act, xshape, n_out):
    def make(dt, dev):
        lin, x = dense_case(act, xshape, n_out, dt, dev, margin=MARGIN_F32)
        return [x, lin.weight, lin.bias], lambda *_: lin(x)
    twin_check("DenseLayer", make, ["zs_dense_act_bwd"] if act else ["zs_column_sum"])


@pytest.mark.gpu
def test_f32_logjoint_scalar_against_f64():
    B, X, H, z_dims = 3, 6, 5, (2, 3)
    rs = np.random.RandomState(9)
    xb = rs.uniform(size=(B, X)) < 0.5
    eps = [rs.standard_normal((B, zd)).astype(np.float32) for zd in z_dims] * 2

    def make(dt, dev):
        torch.manual_seed(0)
        model = ELBO(_Gen(B, X, z_dims, H), _Var(X, z_dims, H)).to(dt).to(dev)
        x = _t(xb, dt, dev)

        def f(*_):
            with zs.inject_epsilon(eps):
                return model({"x": x})
        return list(model.parameters()), f
    twin_check("LogJointScalar", make, ["zs_logjoint_scalar", "zs_logjoint_scalar_bwd"])


@pytest.mark.gpu
@pytest.mark.parametrize("B,D", [(3, 6), (70, 130)], ids=["small", "several_blocks"])
def test_f32_flow_functions_against_f64(B, D):
    rs0 = np.random.RandomState(B + D)
    mask32, x32, ls32 = rs0.uniform(0.2, 0.8, D), rs0.standard_normal((B, D)), 0.3 * rs0.standard_normal((1, D))
    loc32, sc32, c32 = rs0.standard_normal(D), np.exp(0.3 * rs0.standard_normal(D)), rs0.standard_normal(D)

    def f32_exact(module, dt, dev):          # (initialised in float32 and widened: the same numbers in either precision)
        return module.to(dt).to(dev)

    def mask_coupling(dt, dev):
        torch.manual_seed(1)
        layer = f32_exact(MaskCoupling(mask=_t(mask32, dt, dev), inner_nn=_tanh_net(D, 4, D)), dt, dev)
        x = _t(x32, dt, dev)
        return [x] + list(layer.parameters()), lambda x, *_: layer(x)[0]

    def coupling(dt, dev):
        torch.manual_seed(1)
        layer = f32_exact(Coupling(D, 4, 1, 1), dt, dev)
        layer.in_block[1] = nn.Tanh()           # (no kink: the float32 and float64 runs must take the same branch)
        x = _t(x32, dt, dev)
        return [x] + list(layer.parameters()), lambda x, *_: layer(x, reverse=True)[0]

    def scaling(dt, dev):
        layer = Scaling(D).to(dt).to(dev)
        with torch.no_grad():
            layer.log_scale.copy_(_t(ls32, dt, dev))
        x = _t(x32, dt, dev)
        return [x, layer.log_scale], lambda x, _: layer(x.clone())

    def made(dt, dev):
        torch.manual_seed(2)
        layer = f32_exact(MADE(D, 4, 1, activation="tanh"), dt, dev)
        x = _t(x32, dt, dev)
        return [x] + list(layer.parameters()), lambda x, *_: layer(x)

    def tail(base, kind):
        def make(dt, dev):
            loc, scale = _t(loc32, dt, dev), _t(sc32, dt, dev)
            lat = Normal(mean=loc, std=scale) if base == "normal" else Logistic(loc=loc, scale=scale)
            x, a, c = _t(x32, dt, dev), _t(0.5 + mask32, dt, dev), _t(c32, dt, dev)
            return [x, a, c], lambda x, a, c: FlowDistribution(lat, _Probe(a, c, kind), dtype=dt).log_prob(x)
        return make
    with flow_host.count_launches() as c:
        twin_check("Split", mask_coupling)          # (Split and Merge run in both coupling layers)
        twin_check("Merge", coupling)
        twin_check("Scale", scaling)
        twin_check("MadeAffine", made)
        for base in ("normal", "logistic"):
            for kind in ("scalar", "rows"):
                twin_check("Tail", tail(base, kind))
    assert all(c[n] for n in ("split", "split_bwd", "merge", "merge_bwd", "scale_fwd", "scale_bwd", "made_fwd", "made_bwd", "tail", "tail_bwd"))


@pytest.mark.gpu
def test_f32_ratios_cover_every_function_and_are_reported():
    """Runs last: every finite-difference Function has been compared with its float64 twin, and the share of the factor 16
    each one used is printed (``-s``; tests/README.md records a run)."""
    for name, worst in sorted(RATIOS.items()):
        print("%-28s %.2f of 16" % (name, worst))
    if len(RATIOS) > 3:          # (the file's gpu tests ran, not a few selected by hand with -k)
        assert set(RATIOS) == COVERED_BY_FINITE_DIFFERENCES, set(RATIOS) ^ COVERED_BY_FINITE_DIFFERENCES
        assert max(RATIOS.values()) <= 16.0
