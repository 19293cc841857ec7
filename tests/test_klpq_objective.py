"""InclusiveKLObjective (alias KLpq), its sleep phase and zhusuan.evaluation.is_loglikelihood through the public interface, on both
back-ends (``kdev``: the torch restatement of tests/klpq_host.py on the host, the kernels of include/zs_klpq.h on the GPU; the
categorical latent's binding is routed alongside).  See tests/README_klpq.md."""
import inspect
import math
import warnings

import pytest
import torch
import torch.distributions as td

import zhusuan as zs
from zhusuan.framework.bn import BayesianNet
from zhusuan.variational import InclusiveKLObjective, KLpq

import cat_host
import host_backend
import host_routing
import klpq_host
import truth
from klpq_host import kdev  # noqa: F401
from truth import held_to_the_rule, seed_all

F32, F64 = torch.float32, torch.float64


# ``kdev`` with the categorical binding routed as well (the model has an onehot_categorical latent)
qdev = host_routing.dev_fixture("qdev", klpq_host.router, cat_host.router)


class Net(BayesianNet):
    def __init__(self, build):
        super().__init__()
        self.build = build

    def forward(self, observed):
        self.observe(observed)
        self.build(self)
        return self


# ------------------------------------------------------------------------------------------------ interface
def test_import_forms_alias_signature_and_defaults():
    import zhusuan.variational as V
    import zhusuan.variational.inclusive_kl as M
    import zhusuan.evaluation as E
    assert KLpq is InclusiveKLObjective and M.KLpq is InclusiveKLObjective and V.InclusiveKLObjective is InclusiveKLObjective
    assert 'InclusiveKLObjective' in V.__all__ and 'KLpq' in V.__all__ and E.__all__ == ['is_loglikelihood']
    p = inspect.signature(InclusiveKLObjective.__init__).parameters
    assert list(p) == ['self', 'generator', 'variational', 'axis', 'estimator', 'model_grad']
    assert p['axis'].default is None and p['estimator'].default == 'importance' and p['model_grad'].default is False
    f = inspect.signature(InclusiveKLObjective.forward).parameters
    assert list(f) == ['self', 'observed', 'reduce_mean'] and f['reduce_mean'].default is True
    for fn in (E.is_loglikelihood, zs.is_loglikelihood):
        s = inspect.signature(fn).parameters
        assert list(s) == ['generator', 'variational', 'observed', 'axis'] and s['axis'].default == 0
    s = inspect.signature(InclusiveKLObjective.sleep_cost).parameters
    assert list(s) == ['self', 'observed_names', 'n_samples'] and s['n_samples'].default is None
    assert "AIS" in E.__doc__ and "out of scope" in E.__doc__
    obj = KLpq(Net(None), Net(None), axis=0)
    assert isinstance(obj, torch.nn.Module) and obj.last_iw_bound is None and obj.last_ess is None
    assert "not been evaluated" in zs.explain(obj)
    with pytest.raises(NotImplementedError):
        KLpq(Net(None), Net(None), axis=0, estimator='sgvb')
    assert KLpq(Net(None), Net(None), axis=0, estimator='rws').estimator == 'rws'


def test_import_zhusuan_does_not_load_the_library():
    import subprocess
    import sys
    from conftest import PKG_ROOT
    code = ("import sys; sys.path.insert(0, %r); import zhusuan; assert 'zhusuan.evaluation' not in sys.modules; "
            "from zhusuan import _klpq_hip; from zhusuan.variational import KLpq; import zhusuan.evaluation; "
            "assert _klpq_hip._LIB is None; print('lazy')" % PKG_ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "lazy" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------ the model of the value checks
# B = 3, K = 5; q: a Bernoulli latent h [H] and an onehot_categorical latent z [N] given x; p: z, h given z, x given (h, z)
MB, MK, MH, MN, MX = 3, 5, 4, 4, 6


def setup(dev, dtype):
    g = truth.gen(300)
    shapes = dict(qh=(MX, MH), qz=(MX, MN), pz=(MN,), ph=(MN, MH), bh=(MH,), pxh=(MH, MX), pxz=(MN, MX), bx=(MX,))
    P = {k: (0.7 * torch.randn(s, generator=g, dtype=F64)).to(dtype).to(dev).requires_grad_(True) for k, s in shapes.items()}
    x = (torch.rand(MB, MX, generator=g) < 0.5).to(dtype).to(dev)
    return P, x


Q_NAMES, P_NAMES = ('qh', 'qz'), ('pz', 'ph', 'bh', 'pxh', 'pxz', 'bx')


def nets(P, dev, K=MK):
    def q(net):
        x = net.observed['x']
        net.bernoulli('h', logits=x @ P['qh'], n_samples=K, group_ndims=1)
        net.onehot_categorical('z', x @ P['qz'], n_samples=K)

    def p(net):
        B = net.observed['x'].shape[-2]
        z = net.onehot_categorical('z', P['pz'].expand(B, MN), n_samples=K)
        h = net.bernoulli('h', logits=z @ P['ph'] + P['bh'], group_ndims=1)
        net.bernoulli('x', logits=h @ P['pxh'] + z @ P['pxz'] + P['bx'], group_ndims=1)
    return Net(p).to(dev), Net(q).to(dev)


def draws_of(var):
    """the draws the last evaluation used, on the CPU"""
    return {n: var.nodes[n].dist.sample_cache.detach().cpu() for n in ('h', 'z')}


def torch_terms(P, x, draws, dtype):
    """(log p, log q), each [K, B], of the same model with torch.distributions on the CPU in `dtype` at the given draws"""
    h, z = draws['h'].to(dtype), draws['z'].to(dtype)
    K = h.shape[0]
    xc = x.detach().cpu().to(dtype)
    logq = td.Bernoulli(logits=xc @ P['qh']).log_prob(h).sum(-1) + td.OneHotCategorical(logits=xc @ P['qz']).log_prob(z)
    logp = td.OneHotCategorical(logits=P['pz'].expand(MB, MN)).log_prob(z)
    logp = logp + td.Bernoulli(logits=z @ P['ph'] + P['bh']).log_prob(h).sum(-1)
    logp = logp + td.Bernoulli(logits=h @ P['pxh'] + z @ P['pxz'] + P['bx']).log_prob(xc[None].expand(K, MB, MX)).sum(-1)
    return logp, logq


def torch_klpq(logp, logq, model_grad):
    """(cost [B], bound [B], ess [B]) with autograd's own softmax, the weights held constant"""
    lw = (logp - logq).detach()
    w = torch.softmax(lw, 0)
    x = logq + logp if model_grad else logq
    return -(w * x).sum(0), torch.logsumexp(lw, 0) - math.log(lw.shape[0]), 1.0 / (w * w).sum(0)


def torch_model(dtype, x, draws, model_grad):
    P, _ = setup("cpu", dtype)
    cost, bound, ess = torch_klpq(*torch_terms(P, x, draws, dtype), model_grad)
    loss = cost.mean()
    return loss, torch.autograd.grad(loss, list(P.values()), allow_unused=True), cost, bound, ess


@pytest.mark.parametrize("model_grad", [False, True])
def test_value_and_gradients_against_the_float64_model(qdev, model_grad):
    P, x = setup(qdev, F32)
    gen, var = nets(P, qdev)
    obj = KLpq(gen, var, axis=0, model_grad=model_grad).to(qdev)
    seed_all(5)
    loss = obj({'x': x})
    grads = torch.autograd.grad(loss, list(P.values()), allow_unused=True)
    draws = draws_of(var)
    l64, g64, _, b64, e64 = torch_model(F64, x, draws, model_grad)
    l32, g32, _, b32, e32 = torch_model(F32, x, draws, model_grad)
    pairs = [("loss", loss, l32, l64), ("last_iw_bound", obj.last_iw_bound, b32, b64), ("last_ess", obj.last_ess, e32, e64)]
    for n, a, b, c in zip(P.keys(), grads, g32, g64):
        if n in P_NAMES and not model_grad:
            assert a is None or float(a.abs().max()) == 0.0, "without model_grad the generator receives no gradient (%s)" % n
            assert c is None or float(c.abs().max()) == 0.0
            continue
        assert a is not None and c is not None, n
        pairs.append((n, a, b, c))
    held_to_the_rule("model_grad=%s" % model_grad, pairs)
    assert "zs_klpq_forward" in zs.explain(obj)
    assert tuple(obj.last_iw_bound.shape) == (MB,) and not obj.last_iw_bound.requires_grad
    ess = obj.last_ess.detach().cpu()
    assert tuple(ess.shape) == (MB,) and bool((ess >= 1 - 1e-6).all()) and bool((ess <= MK + 1e-5).all())


def test_rws_is_importance_bit_for_bit_and_reduce_mean_false_gives_rows(qdev):
    P, x = setup(qdev, F32)
    out = {}
    for est in ('importance', 'rws'):
        gen, var = nets(P, qdev)
        obj = KLpq(gen, var, axis=0, estimator=est, model_grad=True).to(qdev)
        seed_all(6)
        rows = obj({'x': x}, reduce_mean=False)
        assert tuple(rows.shape) == (MB,)
        seed_all(6)
        loss = obj({'x': x})
        out[est] = [rows.detach(), loss.detach(), obj.last_iw_bound, obj.last_ess] + list(torch.autograd.grad(loss, list(P.values())))
    for a, b in zip(out['importance'], out['rws']):
        assert torch.equal(a, b)
    rows, loss = out['rws'][0], out['rws'][1]
    assert abs(float(rows.double().mean()) - float(loss)) <= 4 * 2.0 ** -24 * float(rows.abs().max())


def test_a_reparameterised_latent_raises_and_a_single_sample_warns_once(qdev):
    P, x = setup(qdev, F32)

    def q(net):
        net.normal('z', mean=net.observed['x'] @ P['qz'], std=1.0, n_samples=MK, group_ndims=1)

    def p(net):
        z = net.normal('z', mean=torch.zeros(MB, MN, device=qdev), std=1.0, n_samples=MK, group_ndims=1)
        net.bernoulli('x', logits=z @ P['pxz'] + P['bx'], group_ndims=1)
    with pytest.raises(ValueError, match="is_reparameterized must be false"):
        KLpq(Net(p).to(qdev), Net(q).to(qdev), axis=0).to(qdev)({'x': x})
    # axis=None: upstream's single-sample behaviour, -log q, with one warning per objective
    gen, var = nets(P, qdev, K=None)
    obj = KLpq(gen, var).to(qdev)
    seed_all(7)
    with pytest.warns(UserWarning, match="single sample"):
        loss = obj({'x': x})
    draws = {n: var.nodes[n].dist.sample_cache.detach().cpu()[None] for n in ('h', 'z')}
    P64, _ = setup("cpu", F64)
    logp, logq = [t.detach() for t in torch_terms(P64, x, draws, F64)]
    assert abs(float(loss.detach()) - float(-logq.mean())) <= 1e-5 * (1 + abs(float(logq.mean())))
    assert float((obj.last_iw_bound.cpu().double() - (logp - logq)[0]).abs().max()) <= 1e-4
    assert bool((obj.last_ess == 1).all()) and "single sample" in zs.explain(obj)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        obj({'x': x})          # the second call is silent
    # K = 1 along a given axis is the same thing
    gen, var = nets(P, qdev, K=1)
    obj = KLpq(gen, var, axis=0).to(qdev)
    terms_p = [torch.full((1, MB), -2.0, device=qdev)]
    terms_q = [torch.full((1, MB), -3.0, device=qdev).requires_grad_(True)]
    with pytest.warns(UserWarning, match="single sample"):
        rows = obj.importance(terms_p, terms_q, reduce_mean=False)
    assert tuple(rows.shape) == (MB,) and bool((rows == 3.0).all()) and bool((obj.last_iw_bound == 1.0).all())


# ------------------------------------------------------------------------------------------------ paths and launches
def launch(c):
    """(K, B, terms of p, terms of q, flags) of a recorded forward; for a backward the terms are those that ask for a gradient"""
    if c.name == "forward":
        (terms_p, terms_q, K, B), flags = c.args, dict(dict(model_grad=False, bound_only=False, want_mean=False), **c.kwargs)
        return K, B, len(terms_p), len(terms_q), flags
    (_, _, want_p, want_q, K, B), flags = c.args[:6], dict(dict(model_grad=False, gcost_is_mean=False), **c.kwargs)
    return K, B, sum(map(bool, want_p)), sum(map(bool, want_q)), flags


def test_one_launch_each_way_and_none_for_an_unused_cost(qdev):
    P, x = setup(qdev, F32)
    gen, var = nets(P, qdev)
    obj = KLpq(gen, var, axis=0, model_grad=True).to(qdev)
    with klpq_host.recording() as calls:
        loss = obj({'x': x})
        assert [c.name for c in calls] == ["forward"] and launch(calls[0])[:4] == (MK, MB, 3, 2)
        assert launch(calls[0])[4] == dict(model_grad=True, bound_only=False, want_mean=True)
        loss.backward()
        assert [c.name for c in calls] == ["forward", "backward"]
        assert launch(calls[1])[2:4] == (3, 2) and launch(calls[1])[4] == dict(model_grad=True, gcost_is_mean=True)
        # without model_grad the generator's terms ask for no gradient
        obj = KLpq(gen, var, axis=0).to(qdev)
        obj({'x': x}).backward()
        assert [c.name for c in calls[2:]] == ["forward", "backward"] and launch(calls[3])[2:4] == (0, 2)
        # a cost that did not enter the loss costs no backward launch
        obj({'x': x})
        (obj.last_ess.sum() + obj.last_iw_bound.sum() + P['qh'].sum()).backward()
        assert [c.name for c in calls[4:]] == ["forward"]
        # is_loglikelihood: one launch in the bound-only mode
        zs.is_loglikelihood(gen, var, {'x': x})
        assert [c.name for c in calls[5:]] == ["forward"] and launch(calls[5])[4]["bound_only"]
    print("launches on %s: %s" % (qdev.type, [(c.name,) + launch(c) for c in calls]))


def rand_terms(dev, shapes, seed, dtype=F32):
    g = truth.gen(seed)
    return [(1.5 * torch.randn(s, generator=g, dtype=F64) - 1.0).to(dtype).to(dev).requires_grad_(True) for s in shapes]


def truth_of(tp, tq, axis, model_grad):
    """float64 autograd of the formulas on CPU copies: (cost rows, bound, ess, gradients of every term)"""
    tp64 = [t.detach().cpu().double().requires_grad_(True) for t in tp]
    tq64 = [t.detach().cpu().double().requires_grad_(True) for t in tq]
    lp, lq = sum(tp64[1:], tp64[0]), sum(tq64[1:], tq64[0])
    lw = (lp - lq).detach()
    w = torch.softmax(lw, axis)
    cost = -(w * (lq + lp if model_grad else lq)).sum(axis)
    grads = torch.autograd.grad(cost.mean(), tp64 + tq64, allow_unused=True)
    return cost.detach(), torch.logsumexp(lw, axis) - math.log(lw.shape[axis]), 1.0 / (w * w).sum(axis), grads


def close(a, b, scale=1.0):
    return float((a.detach().cpu().double() - b).abs().max()) <= 64 * 2.0 ** -24 * scale * (1 + float(b.abs().max()))


def test_layouts_explain_names_the_kernel_or_gives_the_reason(kdev):
    obj = KLpq(Net(None), Net(None), axis=0, model_grad=True).to(kdev)
    K, B = 5, 7
    # [K, B], a transposed [B, K] view, a term shared by the batch and one shared by the particles: views, the kernel
    tp = rand_terms(kdev, [(K, B), (B, K), (K, 1)], 1)
    tq = rand_terms(kdev, [(K, B), (1, B)], 2)
    use_p, use_q = [tp[0], tp[1].t(), tp[2]], tq
    loss = obj.importance(use_p, use_q)
    grads = torch.autograd.grad(loss, tp + tq)
    assert "zs_klpq_forward" in zs.explain(obj) and "because" not in zs.explain(obj)
    cost, bound, ess, g64 = truth_of([tp[0], tp[1].t(), tp[2]], tq, 0, True)
    assert close(loss, cost.mean()) and close(obj.last_iw_bound, bound) and close(obj.last_ess, ess)
    for a, b, t in zip(grads, g64, tp + tq):          # (the truth's second term is a leaf of the transposed shape)
        assert tuple(a.shape) == tuple(t.shape) and close(a, b if b.shape == a.shape else b.t())
    rows = obj.importance(use_p, use_q, reduce_mean=False)
    assert tuple(rows.shape) == (B,) and close(rows, cost)
    # the particle axis last of a 2-D tensor is a layout like any other
    last = KLpq(Net(None), Net(None), axis=-1, model_grad=True).to(kdev)
    rows_t = last.importance([t.t() for t in use_p], [t.t() for t in use_q], reduce_mean=False)
    assert "zs_klpq_forward" in zs.explain(last) and torch.equal(rows_t, rows) and torch.equal(last.last_ess, obj.last_ess)
    # more axes: [K, 2, 3] and a term shared along one batch axis
    tp3, tq3 = rand_terms(kdev, [(K, 2, 3), (K, 1, 3)], 3), rand_terms(kdev, [(K, 2, 3)], 4)
    rows = obj.importance(tp3, tq3, reduce_mean=False)
    cost, bound, ess, _ = truth_of(tp3, tq3, 0, True)
    assert "zs_klpq_forward" in zs.explain(obj) and tuple(rows.shape) == (2, 3) and close(rows, cost) and close(obj.last_iw_bound, bound)
    # a non-zero axis of a 3-D tensor: the torch composition, and explain says why
    mid = KLpq(Net(None), Net(None), axis=1).to(kdev)
    tp3, tq3 = rand_terms(kdev, [(2, K, 3)], 5), rand_terms(kdev, [(2, K, 3)], 6)
    rows = mid.importance(tp3, tq3, reduce_mean=False)
    cost, bound, ess, g64 = truth_of(tp3, tq3, 1, False)
    text = zs.explain(mid)
    assert "torch composition" in text and "because" in text and "particle axis is not 0" in text and "zs_klpq" not in text
    assert tuple(rows.shape) == (2, 3) and close(rows, cost) and close(mid.last_iw_bound, bound) and close(mid.last_ess, ess)
    g, = torch.autograd.grad(rows.mean(), tq3)
    assert close(g, g64[1])
    # more terms than a side takes: the first ones are added with torch, the kernel runs, explain says so
    n = 11
    tp = rand_terms(kdev, [(K, B)] * n, 7)
    loss = obj.importance(tp, tq)
    grads = torch.autograd.grad(loss, tp + tq)
    text = zs.explain(obj)
    assert "zs_klpq_forward" in text and "more than 8 terms" in text and "first 4" in text
    cost, bound, ess, g64 = truth_of(tp, tq, 0, True)
    assert close(loss, cost.mean(), n) and close(obj.last_iw_bound, bound, n)
    for a, b in zip(grads, g64):
        assert close(a, b)
    # equal weights: the effective sample size is K
    same = [torch.zeros(K, B, device=kdev)], [torch.full((K, B), -1.0, device=kdev).requires_grad_(True)]
    obj.importance(*same)          # (1 / 5 is no float32 number: K up to the kernel test's bound for ess, K (2 r + (K + 4) u) with r = (8 + K) u)
    assert float((obj.last_ess - K).abs().max()) <= K * (3 * K + 20) * 2.0 ** -24
    # mixed dtypes: the torch composition
    obj.importance([torch.zeros(K, B, device=kdev, dtype=F64)], same[1])
    assert "torch composition" in zs.explain(obj) and "float32 or all float64" in zs.explain(obj)


def test_a_batch_beyond_one_workgroup_takes_the_rows_and_torchs_mean(kdev):
    K, B = 3, 1025
    obj = KLpq(Net(None), Net(None), axis=0).to(kdev)
    tp, tq = rand_terms(kdev, [(K, B)], 8), rand_terms(kdev, [(K, B)], 9)
    loss = obj.importance(tp, tq)
    g, = torch.autograd.grad(loss, tq)
    cost, _, _, g64 = truth_of(tp, tq, 0, False)
    assert close(loss, cost.mean()) and close(g, g64[1])


# ------------------------------------------------------------------------------------------------ related functions
def test_sleep_cost_against_its_float64_counterpart(qdev):
    P, x = setup(qdev, F32)
    gen, var = nets(P, qdev)
    gen.n_samples = var.n_samples = None          # (these nets fix their K in the closure; the attribute is what sleep_cost sets)

    def p(net):          # nothing observed: the generator's batch comes from its own setting
        z = net.onehot_categorical('z', P['pz'].expand(MB, MN), n_samples=net.n_samples)
        h = net.bernoulli('h', logits=z @ P['ph'] + P['bh'], group_ndims=1)
        net.bernoulli('x', logits=h @ P['pxh'] + z @ P['pxz'] + P['bx'], group_ndims=1)
    gen.build = p
    obj = KLpq(gen, var, axis=0).to(qdev)
    for n_samples in (None, 4):
        seed_all(9)
        loss = obj.sleep_cost(['x'], n_samples=n_samples)
        assert gen.n_samples is None and var.n_samples is None
        grads = torch.autograd.grad(loss, list(P.values()), allow_unused=True)
        dream = {n: var.observed[n].detach().cpu() for n in ('h', 'z', 'x')}
        assert tuple(dream['x'].shape) == ((MB, MX) if n_samples is None else (n_samples, MB, MX))
        res = {}
        for dtype in (F32, F64):
            Pc, _ = setup("cpu", dtype)
            xd, h, z = dream['x'].to(dtype), dream['h'].to(dtype), dream['z'].to(dtype)
            logq = td.Bernoulli(logits=xd @ Pc['qh']).log_prob(h).sum(-1) + td.OneHotCategorical(logits=xd @ Pc['qz']).log_prob(z)
            lc = -logq.mean()
            res[dtype] = (lc, torch.autograd.grad(lc, [Pc[n] for n in Q_NAMES]))
            mag = (td.Bernoulli(logits=xd @ Pc['qh']).log_prob(h).abs().sum(-1) + td.OneHotCategorical(logits=xd @ Pc['qz']).log_prob(z).abs()).mean()
        # the value, one number: a mean over n rows of sums of MH + 1 element terms, each within a few units of float32 --
        # (16 + MH + n) 2^-24 mean_rows sum |terms|  (the 16 x rule on one number hangs on how lucky torch's own float32 sum is)
        n_rows = MB * (n_samples or 1)
        err = abs(float(loss.detach()) - float(res[F64][0]))
        print("sleep cost: error %.3e, bound %.3e" % (err, (16 + MH + n_rows) * 2.0 ** -24 * float(mag)))
        assert err <= (16 + MH + n_rows) * 2.0 ** -24 * float(mag)
        pairs = []
        for i, n in enumerate(Q_NAMES):
            pairs.append((n, grads[list(P.keys()).index(n)], res[F32][1][i], res[F64][1][i]))
        held_to_the_rule("sleep_cost n_samples=%s" % n_samples, pairs)
        for n in P_NAMES:
            a = grads[list(P.keys()).index(n)]
            assert a is None or float(a.abs().max()) == 0.0, "the sleep phase trains q only"
    with pytest.raises(ValueError, match="no node named"):
        obj.sleep_cost(['y'])


def test_is_loglikelihood_is_the_bound_of_the_same_draws_without_a_graph(qdev):
    P, x = setup(qdev, F32)
    gen, var = nets(P, qdev)
    obj = KLpq(gen, var, axis=0).to(qdev)
    seed_all(10)
    obj({'x': x})
    bound = obj.last_iw_bound
    seed_all(10)
    ll = zs.is_loglikelihood(gen, var, {'x': x}, axis=0)
    assert tuple(ll.shape) == (MB,) and not ll.requires_grad and ll.grad_fn is None
    assert torch.equal(ll, bound)
    _, _, _, b64, _ = torch_model(F64, x, draws_of(var), False)
    assert close(ll, b64)
    from zhusuan.evaluation import is_loglikelihood
    seed_all(10)
    assert torch.equal(is_loglikelihood(gen, var, {'x': x}), ll)


def test_is_loglikelihood_accepts_a_reparameterised_normal_latent(qdev):
    P, x = setup(qdev, F32)

    def q(net):
        net.normal('z', mean=net.observed['x'] @ P['qz'], std=1.0, n_samples=MK, group_ndims=1)

    def p(net):
        z = net.normal('z', mean=torch.zeros(MB, MN, device=qdev), std=1.0, n_samples=MK, group_ndims=1)
        net.bernoulli('x', logits=z @ P['pxz'] + P['bx'], group_ndims=1)
    gen, var = Net(p).to(qdev), Net(q).to(qdev)
    seed_all(11)
    ll = zs.is_loglikelihood(gen, var, {'x': x})
    assert tuple(ll.shape) == (MB,) and ll.grad_fn is None and bool(torch.isfinite(ll).all())
    z = var.nodes['z'].dist.sample_cache.detach().cpu().double()
    P64, _ = setup("cpu", F64)
    xc = x.detach().cpu().double()
    logq = td.Normal(xc @ P64['qz'], 1.0).log_prob(z).sum(-1)
    logp = td.Normal(torch.zeros(MB, MN, dtype=F64), 1.0).log_prob(z).sum(-1)
    logp = logp + td.Bernoulli(logits=z @ P64['pxz'] + P64['bx']).log_prob(xc[None].expand(MK, MB, MX)).sum(-1)
    assert close(ll, (torch.logsumexp(logp - logq, 0) - math.log(MK)).detach())


# ------------------------------------------------------------------------------------------------ gpu only
@pytest.mark.gpu
@pytest.mark.parametrize("K,B,model_grad,want_mean", [(1, 2, False, True), (3, 2, True, False), (65, 2, True, True), (65, 2, False, False)])
def test_gradcheck_of_the_f64_function(K, B, model_grad, want_mean):
    """Finite differences of the kernel's own forward against the kernel's backward.  The Function holds the weights constant, as
    upstream's stop_gradient does, so the part of the total derivative that goes through the weights is added back by a term whose
    value is exactly zero (autograd's softmax minus its own detached copy)."""
    from zhusuan.variational._klpq_functions import InclusiveKL
    klpq_host.uninstall()
    dev = torch.device("cuda:0")
    g = truth.gen(K + B)
    tp = [torch.randn(K, B, generator=g, dtype=F64).to(dev).requires_grad_(True), torch.randn(B, K, generator=g, dtype=F64).to(dev).requires_grad_(True)]
    tq = [torch.randn(K, B, generator=g, dtype=F64).to(dev).requires_grad_(True), torch.randn(1, B, generator=g, dtype=F64).to(dev).requires_grad_(True)]

    def f(p0, p1, q0, q1):
        terms = [p0, p1.t(), q0, q1]
        cost, _, _ = InclusiveKL.apply(K, B, 2, model_grad, want_mean, *terms)
        lp, lq = p0 + p1.t(), q0 + q1
        w = torch.softmax(lp - lq, 0)
        x = (lq + lp if model_grad else lq).detach()
        through_w = -((w - w.detach()) * x).sum(0)
        return cost + (through_w.mean() if want_mean else through_w)
    assert torch.autograd.gradcheck(f, tp + tq, eps=1e-6, atol=1e-7, rtol=1e-5, nondet_tol=0.0)


@pytest.mark.gpu
def test_inside_graphedstep_the_cost_changes_from_replay_to_replay_and_training_proceeds():
    from examples import rws_sbn as E
    klpq_host.uninstall()
    cat_host.uninstall()
    host_backend.uninstall()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = E.build('rws', 'bernoulli', x_dim=16, h1=8, h2=4, n_samples=5, batch=8, device=dev)
    x = E.synthetic_data(8, 16).to(dev)
    opt = torch.optim.Adam(model.parameters(), 1e-2, capturable=True)
    rng = zs.DeviceRNG(dev, seed=12)
    before = [p.detach().clone() for p in model.parameters()]

    def compute():
        rng.begin_step()
        loss = model({'x': x})
        opt.zero_grad(set_to_none=True)
        loss.backward()
        return loss.detach()
    step = zs.GraphedStep(compute, optimizer_step=opt.step, rng=rng, warmup=3)
    assert step.captured, step.capture_error
    losses = []
    for _ in range(4):
        losses.append(step().clone())
    torch.cuda.synchronize()
    vals = [float(v) for v in losses]
    assert all(math.isfinite(v) for v in vals) and len(set(vals)) == len(vals), vals
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, model.parameters()))
    assert "zs_klpq_forward" in zs.explain(model)
