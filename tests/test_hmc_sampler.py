"""``zhusuan.mcmc.HMC`` at the level of its public interface, on both back-ends of the suite's ``dev`` fixture: "hip" is the
package on libzs_hmc.so, "host" the same package code with the three functions of the binding replaced by the torch
restatements of tests/hmc_host.py (and the other kernels by the C oracle, tests/host_backend.py).  The truth is the pure
float64 iteration of tests/hmc_host.py, and properties that any correct HMC has."""
import inspect
import math

import pytest
import torch

import hmc_host
import host_backend
import truth
from hmc_host import hdev  # noqa: F401
from truth import seed_all

F32, F64 = torch.float32, torch.float64


# ------------------------------------------------------------------------------------------------ models
def density_net(dev, fn):
    """A BayesianNet whose log joint is ``fn(observed)``, per chain: the form of the reference's own sampler test
    (test/mcmc/test_mcmc.py overrides ``_log_joint``)."""
    from zhusuan.framework.bn import BayesianNet

    class Net(BayesianNet):
        def forward(self, observed):
            self.observe(observed)
            return self

        def _log_joint(self):
            return fn(self.observed)
    return Net().to(dev)


def quartic(dev):
    return density_net(dev, lambda o: 2 * o['x'] ** 2 - o['x'] ** 4)


def gaussian(dev, std):
    std = std.to(dev)
    return density_net(dev, lambda o: (-0.5 * (o['x'] / std) ** 2).sum(-1))


N_DATA = 6


def blr_data(C, dtype=F32):
    gen = truth.gen(40)
    x = torch.randn(N_DATA, 5, generator=gen, dtype=F64)
    y = (x.sum(1) * 0.3 + 0.2 * torch.randn(N_DATA, generator=gen, dtype=F64))
    return x.to(dtype), y.to(dtype).unsqueeze(0).expand(C, N_DATA).contiguous()


def blr_net(dev, C, dtype=F32):
    """Bayesian linear regression as a BayesianNet: w ~ Normal [C, 5], a second latent b ~ Normal [C, 2, 3] whose sum shifts
    the mean, a Normal likelihood; ``group_ndims`` make the log joint [C]."""
    from zhusuan.framework.bn import BayesianNet

    class Net(BayesianNet):
        def forward(self, observed):
            self.observe(observed)
            w = self.normal('w', mean=torch.zeros([C, 5], dtype=dtype, device=dev), std=torch.ones([C, 5], dtype=dtype, device=dev),
                            group_ndims=1)
            b = self.normal('b', mean=torch.zeros([C, 2, 3], dtype=dtype, device=dev),
                            std=torch.full([C, 2, 3], 2.0, dtype=dtype, device=dev), group_ndims=2)
            mean = torch.matmul(w, self.observed['x'].t()) + 0.1 * b.sum((1, 2)).unsqueeze(1)
            self.normal('y', mean=mean, std=torch.full([C, N_DATA], 0.5, dtype=dtype, device=dev), group_ndims=1)
            return self
    return Net().to(dev)


def blr_logp_and_grad(x, y):
    """The same density in plain torch, in the dtype of the tensors given."""
    def f(qs):
        w, b = [t.detach().requires_grad_(True) for t in qs]
        c = -0.5 * math.log(2 * math.pi)
        lp = (c - 0.5 * w ** 2).sum(1) + (c - math.log(2.0) - 0.5 * (b / 2.0) ** 2).sum((1, 2))
        mean = torch.matmul(w, x.to(w.dtype).t()) + 0.1 * b.sum((1, 2)).unsqueeze(1)
        lp = lp + (c - math.log(0.5) - 0.5 * ((y.to(w.dtype) - mean) / 0.5) ** 2).sum(1)
        return lp.detach(), list(torch.autograd.grad(lp.sum(), [w, b]))
    return f


def independent_normals(dev, k, C, dtype=F32, mean=0.5, std=2.0):
    """k latent nodes z0 .. z{k-1} of [C, 1 .. 5] elements, N(mean, std^2) each."""
    from zhusuan.framework.bn import BayesianNet

    class Net(BayesianNet):
        def forward(self, observed):
            self.observe(observed)
            for i in range(k):
                n = 1 + i % 5
                self.normal('z%d' % i, mean=torch.full([C, n], mean, dtype=dtype, device=dev),
                            std=torch.full([C, n], std, dtype=dtype, device=dev), group_ndims=1)
            return self
    return Net().to(dev)


class Counted(object):
    """Wraps the three functions of the binding (whichever are installed), ``_rng.next_call`` and a net's forward."""

    def __init__(self, net=None):
        self.net = net

    def __enter__(self):
        from zhusuan import _hmc_hip, _rng
        self.mods = (_hmc_hip, _rng)
        self.inner = (_hmc_hip.move, _hmc_hip.decide, _hmc_hip.select, _rng.next_call)
        self.moves, self.decides, self.selects, self.ids, self.forwards = [], [], [], [], 0

        def move(kind, n_chains, state, q, *a, **kw):
            self.moves.append((kind, len(q)))
            return self.inner[0](kind, n_chains, state, q, *a, **kw)

        def decide(chunks, *a, **kw):
            self.decides.append(len(chunks))
            self.ids.append(("uniform", kw.get("call")))
            return self.inner[1](chunks, *a, **kw)

        def select(n_chains, q0, *a, **kw):
            self.selects.append(len(q0))
            return self.inner[2](n_chains, q0, *a, **kw)

        def next_call(device):
            r = self.inner[3](device)
            self.ids.append(("next_call", r[1]))
            return r
        _hmc_hip.move, _hmc_hip.decide, _hmc_hip.select, _rng.next_call = move, decide, select, next_call
        if self.net is not None:
            fwd = self.net.forward

            def forward(observed):
                self.forwards += 1
                return fwd(observed)
            self.net.forward = forward
        return self

    def __exit__(self, *exc):
        h, r = self.mods
        h.move, h.decide, h.select, r.next_call = self.inner
        if self.net is not None:
            del self.net.forward


# ------------------------------------------------------------------------------------------------ interface
def test_import_forms_signature_and_defaults():
    import zhusuan as zs
    import zhusuan.mcmc
    from zhusuan.mcmc import HMC, HMCInfo
    from zhusuan.mcmc.HMC import HMC as HMC2
    assert HMC is HMC2 and zs.mcmc.HMC is HMC
    sig = inspect.signature(HMC.__init__)
    assert [(k, p.default) for k, p in list(sig.parameters.items())[1:]] == [
        ("step_size", 1.), ("n_leapfrogs", 10), ("adapt_step_size", False), ("target_acceptance_rate", 0.8), ("gamma", 0.05),
        ("t0", 100), ("kappa", 0.75), ("adapt_mass", False)]
    assert list(inspect.signature(HMC.sample).parameters)[1:] == ["bn", "observed", "latent", "inplace"]
    assert inspect.signature(HMC.sample).parameters["inplace"].default is False
    assert HMCInfo._fields == ("samples", "acceptance_rate", "updated_step_size", "init_momentum", "orig_hamiltonian", "hamiltonian",
                               "orig_log_prob", "log_prob")
    h = HMC(step_size=0.01, n_leapfrogs=10)          # the reference's commented-out call
    assert h.t == 0 and h.step_size == 0.01 and h.adapt_step_size is False and h.n_leapfrogs == 10
    h.adapt_step_size = True
    assert h.adapt_step_size is True
    with pytest.raises(NotImplementedError, match="mass adaptation is not implemented"):
        HMC(adapt_mass=True)


@pytest.mark.parametrize("chain_shape", [(), (3,), (2, 3)], ids=["scalar", "C3", "2x3"])
def test_info_fields_shapes_inplace_and_chain_shape_error(hdev, chain_shape):
    from zhusuan.mcmc import HMC
    std = torch.tensor([0.5, 1.0, 2.0])
    net = gaussian(hdev, std)
    seed_all(1, hdev)
    x = torch.randn(*chain_shape, 3).to(hdev)
    kept = x.clone()
    h = HMC(step_size=0.2, n_leapfrogs=3)
    samples, info = h.sample(net, {}, {'x': x})
    assert h.t == 1 and list(samples) == ['x'] and info.samples is samples
    assert torch.equal(x, kept) and samples['x'].data_ptr() != x.data_ptr() and samples['x'].shape == x.shape
    assert not samples['x'].requires_grad and samples['x'].device == x.device
    for f in ("acceptance_rate", "orig_hamiltonian", "hamiltonian", "orig_log_prob", "log_prob"):
        v = getattr(info, f)
        assert tuple(v.shape) == chain_shape and v.device == x.device and bool(torch.isfinite(v).all()), f
    assert info.updated_step_size.dim() == 0 and info.updated_step_size.device == x.device and float(info.updated_step_size) == 0.2
    assert list(info.init_momentum) == ['x'] and info.init_momentum['x'].shape == x.shape
    k0 = 0.5 * (info.init_momentum['x'] ** 2).sum(-1)
    assert torch.allclose(info.orig_hamiltonian, k0 - info.orig_log_prob, rtol=1e-5, atol=1e-6)
    moved = (samples['x'] != x).reshape(-1, 3).any(1).reshape(chain_shape)
    assert torch.equal(torch.where(moved, info.log_prob, info.orig_log_prob), info.log_prob)
    assert bool(((info.acceptance_rate >= 0) & (info.acceptance_rate <= 1)).all())
    # in place: the same objects, written into their storage
    y = x.clone()
    ptr = y.data_ptr()
    seed_all(2, hdev)
    s2, _ = h.sample(net, {}, {'x': y}, inplace=True)
    seed_all(2, hdev)
    s3, _ = h.sample(net, {}, {'x': x})
    assert s2['x'] is y and y.data_ptr() == ptr and torch.equal(y, s3['x']) and h.t == 3
    with pytest.raises(ValueError, match="'x' is not contiguous"):
        h.sample(net, {}, {'x': x.clone().transpose(-1, -2) if x.dim() > 1 else x.repeat(2)[::2]}, inplace=True)
    # a latent whose shape does not begin with the chain shape
    if chain_shape:
        net2 = density_net(hdev, lambda o: (-0.5 * o['x'] ** 2).sum(-1) - 0.5 * o['v'].sum() ** 2)
        with pytest.raises(ValueError, match="latent 'v'"):
            h.sample(net2, {}, {'x': x, 'v': torch.zeros(7, device=hdev)})


# ------------------------------------------------------------------------------------------------ trajectory
TRAJECTORY_SEEDS = {1: 3, 3: 3}
L_TRAJ, EPS_TRAJ, ITERS = 3, 0.05, 4


def trajectory_inputs(C, seed):
    gen = truth.gen(seed)
    q0 = [0.3 * torch.randn(C, 5, generator=gen), 0.3 * torch.randn(C, 2, 3, generator=gen)]
    zs = [[torch.randn(C, 5, generator=gen), torch.randn(C, 2, 3, generator=gen)] for _ in range(ITERS)]
    us = [torch.rand(C, generator=gen) for _ in range(ITERS)]
    return q0, zs, us


def reference_trajectory(C, seed, dtype):
    x, y = blr_data(C)
    f = blr_logp_and_grad(x, y)
    q, zs, us = trajectory_inputs(C, seed)
    q = [t.to(dtype) for t in q]
    out = []
    for z, u in zip(zs, us):
        r = hmc_host.reference_iteration(f, q, [t.to(dtype) for t in z], u, EPS_TRAJ, L_TRAJ)
        r["margin"] = (torch.log(u.double()) - r["dh"]).abs()
        q = r["q"]
        out.append(r)
    return out


@pytest.mark.parametrize("C", [1, 3])
def test_trajectory_matches_the_float64_reference_iteration(hdev, C):
    """Tolerance per quantity: 16 x the distance between the reference iteration run in float32 and in float64 (the golden
    tests' convention).  Measured on the host back-end: see the assertion messages (the product's distance is of the same
    order as the reference's own)."""
    import zhusuan
    from zhusuan.mcmc import HMC
    seed = TRAJECTORY_SEEDS[C]
    r64, r32 = reference_trajectory(C, seed, F64), reference_trajectory(C, seed, F32)
    assert all(float(r["margin"].min()) > 1e-2 for r in r64), "the fixed seed puts a decision within 1e-2 of its threshold"
    x, y = blr_data(C)
    net = blr_net(hdev, C)
    obs = {'x': x.to(hdev), 'y': y.to(hdev)}
    q, zs, us = trajectory_inputs(C, seed)
    latent = {'w': q[0].to(hdev), 'b': q[1].to(hdev)}
    h = HMC(step_size=EPS_TRAJ, n_leapfrogs=L_TRAJ)
    got = []
    for z, u in zip(zs, us):
        with zhusuan.inject_epsilon(z + [u]):
            latent, info = h.sample(net, obs, latent)
        got.append((latent, info))

    def dist(f):
        return max(float((f(a) - f(b)).abs().max()) for a, b in zip(r32, r64))
    quantities = [("w", lambda r: r["q"][0].double(), lambda s, i: s['w']), ("b", lambda r: r["q"][1].double(), lambda s, i: s['b']),
                  ("h0", lambda r: r["h0"], lambda s, i: i.orig_hamiltonian), ("h1", lambda r: r["h1"], lambda s, i: i.hamiltonian),
                  ("a", lambda r: r["a"], lambda s, i: i.acceptance_rate), ("logp0", lambda r: r["logp0"], lambda s, i: i.orig_log_prob)]
    for name, ref, mine in quantities:
        tol = 16 * dist(ref)
        err = max(float((mine(s, i).detach().cpu().double().reshape(ref(r).shape) - ref(r)).abs().max()) for (s, i), r in zip(got, r64))
        assert err <= tol, (name, err, tol)
    for (s, i), r in zip(got, r64):
        decided = (i.log_prob.cpu().double() - r["logp0"]).abs() > 0.5 * (r["logp1"] - r["logp0"]).abs()
        assert torch.equal(decided, r["accept"]), "decisions differ"
    assert h.t == ITERS


# ------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("L", [1, 3, 10])
def test_launch_budget_and_call_ids(hdev, L):
    from zhusuan.mcmc import HMC
    C = 3
    x, y = blr_data(C)
    net = blr_net(hdev, C)
    obs = {'x': x.to(hdev), 'y': y.to(hdev)}
    latent = {'w': torch.zeros(C, 5, device=hdev), 'b': torch.zeros(C, 2, 3, device=hdev)}
    h = HMC(step_size=0.05, n_leapfrogs=L)
    seed_all(3, hdev)
    for it in range(2):
        with Counted(net) as c:
            latent, _ = h.sample(net, obs, latent)
        assert c.moves == [(hmc_host.BEGIN, 2)] + [(hmc_host.STEP, 2)] * (L - 1) + [(hmc_host.END, 2)]
        assert c.decides == [1] and c.selects == [2]
        assert len(c.moves) + len(c.decides) + len(c.selects) == L + 3
        assert c.forwards == L + 1
        kinds = [k for k, _ in c.ids]
        assert kinds == ["next_call", "next_call", "uniform"], "two call ids per iteration: momentum first, uniform second"
        assert c.ids[1][1] == c.ids[2][1] and c.ids[0][1] != c.ids[1][1]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_forty_latents_are_two_chunks_and_one_decide(hdev, dtype):
    """40 independent Normal latents, injected draws, against the float64 reference iteration.  Bound: a leapfrog of three steps
    is about ten roundings per element, 10 x 3 x 2^-24 = 1.8e-6 relative in float32; 1e-5 (1 + |q|) leaves a factor five, and
    2^-29 of that for float64."""
    import zhusuan
    from zhusuan.mcmc import HMC
    k, C, L, eps = 40, 3, 3, 0.3
    net = independent_normals(hdev, k, C, dtype)
    gen = truth.gen(8)
    shapes = [(C, 1 + i % 5) for i in range(k)]
    q0 = [torch.randn(s, generator=gen, dtype=F64).to(dtype) for s in shapes]
    z = [torch.randn(s, generator=gen, dtype=F64).to(dtype) for s in shapes]
    u = torch.rand(C, generator=gen, dtype=F64).to(dtype)
    h = HMC(step_size=eps, n_leapfrogs=L)
    with zhusuan.inject_epsilon(z + [u]):
        with Counted() as c:
            out, info = h.sample(net, {}, dict(('z%d' % i, t.to(hdev)) for i, t in enumerate(q0)))
    assert c.moves == [(kind, n) for kind in (hmc_host.BEGIN, hmc_host.STEP, hmc_host.STEP, hmc_host.END) for n in (32, 8)]
    assert c.decides == [2] and c.selects == [32, 8]
    assert list(out) == ['z%d' % i for i in range(k)]

    def f(qs):
        qs = [t.detach().requires_grad_(True) for t in qs]
        lp = sum((-0.5 * math.log(2 * math.pi) - math.log(2.0) - 0.5 * ((t - 0.5) / 2.0) ** 2).sum(1) for t in qs)
        return lp.detach(), list(torch.autograd.grad(lp.sum(), qs))
    r = hmc_host.reference_iteration(f, [t.double() for t in q0], [t.double() for t in z], u.double(), eps, L)
    assert float((torch.log(u.double()) - r["dh"]).abs().min()) > 1e-3
    rel = 1e-5 if dtype == F32 else 1e-5 * 2.0 ** -29
    for i in range(k):
        got = out['z%d' % i].cpu()
        assert got.dtype == dtype and bool(((got.double() - r["q"][i]).abs() <= rel * (1 + r["q"][i].abs())).all()), i
    assert bool(((info.hamiltonian.cpu().double() - r["h1"]).abs() <= 20 * rel * (1 + r["h1"].abs())).all())


def test_chain_independence(hdev):
    """Changing the inputs of the other chains leaves chain 0's sample bit-identical."""
    import zhusuan
    from zhusuan.mcmc import HMC
    C = 3
    x, y = blr_data(C)
    net = blr_net(hdev, C)
    obs = {'x': x.to(hdev), 'y': y.to(hdev)}
    q, zs, us = trajectory_inputs(C, 11)

    def run(change):
        qq = [t.clone() for t in q]
        z = [t.clone() for t in zs[0]]
        u = us[0].clone()
        if change:
            for t in qq + z:
                t[1:] = t[1:] * -1.5 + 0.25
            qq[0][2] = 1e4                      # a chain far out: a huge energy error, rejected on its own
            u[1:] = 1.0 - u[1:]
        with zhusuan.inject_epsilon(z + [u]):
            s, i = HMC(step_size=0.05, n_leapfrogs=4).sample(net, obs, {'w': qq[0].to(hdev), 'b': qq[1].to(hdev)})
        return s, i
    (a, ia), (b, ib) = run(False), run(True)
    for k in a:
        assert torch.equal(a[k][0], b[k][0]) and not torch.equal(a[k][1:], b[k][1:])
    assert torch.equal(ia.hamiltonian[0], ib.hamiltonian[0]) and torch.equal(ia.acceptance_rate[0], ib.acceptance_rate[0])


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_reversibility_through_the_move_entry_points(hdev, dtype):
    """L steps, negate p, L steps returns to q0 within 32 ulp (1 + max|q|).  A torch restatement on the CPU measured
    0.55 x 2^-23 (1 + max|q|) in float32 on this problem (7-dimensional Gaussian, L = 10, eps = 0.1)."""
    from zhusuan import _hmc_hip
    C, D, L, eps = 5, 7, 10, 0.1
    std = torch.linspace(0.5, 2.0, D, dtype=F64).to(dtype).to(hdev)
    gen = truth.gen(2)
    q0 = (torch.randn(C, D, generator=gen, dtype=F64) * std.cpu().double()).to(dtype).to(hdev)
    z = torch.randn(C, D, generator=gen, dtype=F64).to(dtype).to(hdev)
    state = torch.tensor([eps, eps, 0, 0, 0, 0, 0, 0], dtype=F64, device=hdev)
    ksum = torch.empty(C * _hmc_hip.ksum_slots([D]), dtype=dtype, device=hdev)

    def grad(q):
        return (-q / (std * std)).contiguous()

    def trajectory(start, mom):
        q, p = torch.empty_like(start), torch.empty_like(start)
        _hmc_hip.move(_hmc_hip.BEGIN, C, state, [q], [p], [grad(start)], q0=[start], z=[mom], ksum=ksum)
        for _ in range(L - 1):
            _hmc_hip.move(_hmc_hip.STEP, C, state, [q], [p], [grad(q)])
        return q, p + 0.5 * eps * grad(q)
    qL, pL = trajectory(q0, z)
    back, _ = trajectory(qL, (-pL).contiguous())
    ulp = 2.0 ** -23 if dtype == F32 else 2.0 ** -52
    qmax = max(float(q0.abs().max()), float(qL.abs().max()))
    err = float((back - q0).abs().max())
    assert float((qL - q0).abs().max()) > 0.1 and err <= 32 * ulp * (1 + qmax), (err / (ulp * (1 + qmax)))


def test_energy_error_is_second_order(hdev):
    """float64, a 7-dimensional Gaussian with standard deviations 0.5 .. 2, 65 chains: max |dH| at (eps, L) = (0.1, 10) over
    that at (0.05, 20) lies in [3.5, 4.5] (a torch restatement gives 4.03)."""
    import zhusuan
    from zhusuan.mcmc import HMC
    C, D = 65, 7
    std = torch.linspace(0.5, 2.0, D, dtype=F64)
    net = gaussian(hdev, std)
    gen = truth.gen(6)
    q0 = (torch.randn(C, D, generator=gen, dtype=F64) * std).to(hdev)
    z = torch.randn(C, D, generator=gen, dtype=F64)
    u = torch.rand(C, generator=gen, dtype=F64)
    worst = []
    for eps, L in [(0.1, 10), (0.05, 20)]:
        with zhusuan.inject_epsilon([z, u]):
            _, info = HMC(step_size=eps, n_leapfrogs=L).sample(net, {}, {'x': q0})
        worst.append(float((info.hamiltonian - info.orig_hamiltonian).abs().max()))
    assert 3.5 <= worst[0] / worst[1] <= 4.5, worst


# ------------------------------------------------------------------------------------------------ correct target
def quartic_moments():
    """m2 and m4 of p(x) ~ exp(2 x^2 - x^4) by float64 quadrature (Simpson, 40001 nodes on [-6, 6])."""
    x = torch.linspace(-6.0, 6.0, 40001, dtype=F64)
    w = torch.ones_like(x)
    w[1:-1:2], w[2:-1:2] = 4.0, 2.0
    d = w * torch.exp(2 * x ** 2 - x ** 4)
    return float((d * x ** 2).sum() / d.sum()), float((d * x ** 4).sum() / d.sum())


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_samples_the_reference_tests_density(hdev, dtype):
    """log p(x) = 2 x^2 - x^4 (the reference test's density without its noise term), 4096 chains from x = 0, eps = 0.1, L = 10,
    100 iterations, through the commented-out test's calling convention.  A float64 torch HMC with these settings stayed
    within 2.5 standard errors on both statistics for six seeds; the host back-end with seed 3 gives mean -0.011 and
    mean(x^2) 0.836 against bounds 0.071 and 0.049."""
    from zhusuan.mcmc import HMC
    m2, m4 = quartic_moments()
    assert abs(m2 - 0.83275) < 1e-5 and abs(m4 - 1.08275) < 1e-5
    n = 4096
    net = quartic(hdev)
    x = torch.zeros(n, dtype=dtype, device=hdev)
    sampler = HMC(step_size=0.1, n_leapfrogs=10)
    seed_all(3, hdev)
    rate = 0.0
    for _ in range(100):
        info = sampler.sample(net, {}, {'x': x}, inplace=True)[1]
        rate = rate + info.acceptance_rate.mean()
    xs = x.double().cpu()
    assert bool(torch.isfinite(xs).all()) and float(rate) / 100 > 0.97
    assert abs(float(xs.mean())) <= 5 * math.sqrt(m2 / n), float(xs.mean())
    assert abs(float((xs ** 2).mean()) - m2) <= 5 * math.sqrt((m4 - m2 ** 2) / n), float((xs ** 2).mean())


# ------------------------------------------------------------------------------------------------ adaptation
def test_step_size_adaptation_from_both_sides(hdev):
    """A 10-dimensional Gaussian with standard deviations 0.5 .. 2, 256 chains, L = 5, float64; 300 adapting iterations, then
    100 frozen, from step_size 0.01 and from 5.0.  Measured with the host back-end (seed 5): frozen step sizes 0.6635 and 0.6666
    (0.5 % apart; threshold 5 %), frozen mean acceptance 0.801 and 0.795 (threshold 0.05 around 0.8); the issue's float64
    restatement gave 0.663 - 0.667 and 0.795 - 0.804 across four seeds.  The run from 5.0 starts far beyond the stability limit
    (energy errors of 1e30 and more, every chain rejected); non-finite energies themselves are the subject of
    test_non_finite_energies_reject_only_their_chain."""
    from zhusuan.mcmc import HMC
    std = torch.linspace(0.5, 2.0, 10, dtype=F64)
    net = gaussian(hdev, std)
    frozen, rates, first_rates = [], [], []
    for e0 in (0.01, 5.0):
        seed_all(5, hdev)
        h = HMC(step_size=e0, n_leapfrogs=5, adapt_step_size=True)
        latent = {'x': torch.zeros(256, 10, dtype=F64, device=hdev)}
        for it in range(300):
            latent, info = h.sample(net, {}, latent)
            if it == 0:
                first_rates.append(info.acceptance_rate.mean())
        h.adapt_step_size = False
        rate = 0.0
        for _ in range(100):
            latent, info = h.sample(net, {}, latent)
            rate = rate + info.acceptance_rate.mean()
            step = info.updated_step_size
        assert h.t == 400 and bool(torch.isfinite(latent['x']).all())
        assert float(step) == h.step_size, "the frozen step size moved"
        frozen.append(h.step_size)
        rates.append(float(rate) / 100)
    assert float(first_rates[0]) > 0.99 and float(first_rates[1]) < 1e-6
    assert abs(frozen[0] - frozen[1]) <= 0.05 * min(frozen), frozen
    assert all(abs(r - 0.8) <= 0.05 for r in rates), rates


def test_non_finite_energies_reject_only_their_chain(hdev):
    """float32, the quartic density: a chain at 1e20 has log joint inf - inf = NaN, one at 3e9 a finite log joint and an
    infinite one after a step.  Both stay where they are, iteration after iteration; the other chains move, the step size
    adapts from finite numbers."""
    from zhusuan.mcmc import HMC
    net = quartic(hdev)
    x = torch.zeros(64, device=hdev)
    x[5], x[9] = 1e20, 3e9
    kept = x.clone()
    h = HMC(step_size=0.1, n_leapfrogs=4, adapt_step_size=True)
    seed_all(9, hdev)
    for _ in range(5):
        _, info = h.sample(net, {}, {'x': x}, inplace=True)
        assert float(info.acceptance_rate[5]) == 0.0 and float(info.acceptance_rate[9]) == 0.0
    ok = torch.ones(64, dtype=torch.bool, device=hdev)
    ok[5] = ok[9] = False
    assert torch.equal(x[~ok], kept[~ok])
    assert bool(torch.isfinite(x[ok]).all()) and bool((x[ok] != 0).all())
    assert bool(torch.isfinite(info.acceptance_rate).all()) and math.isfinite(h.step_size) and 0.01 < h.step_size < 10.0


# ------------------------------------------------------------------------------------------------ gpu only
def _run(dev, iters=3, rng=None):
    import zhusuan
    from zhusuan.mcmc import HMC
    C = 3
    x, y = blr_data(C)
    net = blr_net(dev, C)
    obs = {'x': x.to(dev), 'y': y.to(dev)}
    latent = {'w': torch.zeros(C, 5, device=dev), 'b': torch.zeros(C, 2, 3, device=dev)}
    h = HMC(step_size=0.05, n_leapfrogs=3)
    out = []
    for _ in range(iters):
        if rng is not None:
            rng.begin_step()
            with zhusuan.device_rng(rng):
                latent, info = h.sample(net, obs, latent)
        else:
            latent, info = h.sample(net, obs, latent)
        out.append(torch.cat([latent['w'].flatten(), latent['b'].flatten(), info.acceptance_rate]).cpu())
    return out


@pytest.mark.gpu
def test_seeds_and_device_rng_reproduce_a_run():
    import zhusuan
    dev = torch.device("cuda:0")
    host_backend.uninstall()
    hmc_host.uninstall()
    torch.cuda.manual_seed(21)
    a = _run(dev)
    torch.cuda.manual_seed(21)
    b = _run(dev)
    torch.cuda.manual_seed(22)
    c = _run(dev)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not any(torch.equal(x, y) for x, y in zip(a, c))
    d = _run(dev, rng=zhusuan.DeviceRNG(dev, seed=7))
    e = _run(dev, rng=zhusuan.DeviceRNG(dev, seed=7))
    f = _run(dev, rng=zhusuan.DeviceRNG(dev, seed=8))
    assert all(torch.equal(x, y) for x, y in zip(d, e)) and not any(torch.equal(x, y) for x, y in zip(d, f))
    assert not torch.equal(d[0], d[1])


@pytest.mark.gpu
def test_a_host_tensor_raises():
    from zhusuan.mcmc import HMC
    host_backend.uninstall()
    hmc_host.uninstall()
    net = quartic(torch.device("cpu"))
    with pytest.raises(RuntimeError, match="no CPU path|HIP device"):
        HMC(step_size=0.1, n_leapfrogs=2).sample(net, {}, {'x': torch.zeros(4)})


@pytest.mark.gpu
def test_missing_library_names_the_build_command_and_leaves_the_rest_working(tmp_path, monkeypatch):
    from zhusuan import _hmc_hip
    from zhusuan.mcmc import HMC, SGLD
    dev = torch.device("cuda:0")
    host_backend.uninstall()
    hmc_host.uninstall()
    missing = str(tmp_path / "libzs_hmc.so")
    with pytest.raises(RuntimeError, match="make -C zhusuan-pytorch_amd/csrc hmc"):
        _hmc_hip.lib(missing)
    monkeypatch.setattr(_hmc_hip, "LIB_PATH", missing)
    monkeypatch.setattr(_hmc_hip, "_LIB", None)
    net = quartic(dev)
    x = torch.zeros(8, device=dev)
    with pytest.raises(RuntimeError, match="make -C zhusuan-pytorch_amd/csrc hmc"):
        HMC(step_size=0.1, n_leapfrogs=2).sample(net, {}, {'x': x})
    assert bool((x == 0).all())
    # the stochastic-gradient samplers run on their own library
    import mcmc_models as M
    from zhusuan.framework.bn import BayesianNet
    xd, yd = M.make_data(3, 3)
    bn = M.make_net(BayesianNet, [3, 4, 1], device=dev)
    obs = {'x': torch.tensor(xd, device=dev), 'y': torch.tensor(yd, device=dev)}
    s = SGLD(1e-3)
    s.sample(bn, obs, resample=True)
    assert bool(torch.isfinite(s.sample(bn, obs)['w0']).all())
