"""Which Philox (seed, call id) pairs the package hands to its libraries, on both back-ends (tests/README_rng.md).

Two launches that resolve to the same pair draw identical noise for two latents: values stay finite and nothing else
notices.  ``Recorder`` wraps the layer where the package calls its libraries (``KernelLibrary.call`` of the main library,
``_mcmc_hip.update``, ``_hmc_hip.move`` / ``decide`` -- whichever functions are installed, so the host back-end too) and keeps
for every launch that draws the entry point, the resolved ids and whether it is a forward draw or a backward
regeneration; a device-resident ``rng_state`` is resolved through its value at the call.  The package is not changed.
Hipgraph replays are not intercepted (tests/test_graph.py pins fresh draws per replay)."""
import contextlib

import numpy as np
import pytest
import torch

import flow_host
import helpers as H
import hmc_host
import host_backend
import host_routing
import mcmc_host
import zhusuan as zs
from zhusuan import _hip, _ops, _rng
from zhusuan.framework.bn import BayesianNet
from zhusuan.variational.elbo import ELBO

M64 = 2 ** 64 - 1
SEED = 67280421310721 + 2 ** 40          # upper word non-zero, as every seed of torch.seed() and torch's default
STEPS = 3


ROUTERS = (mcmc_host.router, hmc_host.router, flow_host.router)
# the suite's ``dev`` with every sampler / flow binding routed like the main library
adev = host_routing.dev_fixture("adev", *ROUTERS)


# ------------------------------------------------------------------------------------------------ recording
# entry point (without _f32 / _f64) -> (index of the operand whose absence means "the kernel draws", or None; index of seed)
# the argument order is that of include/zs_hip.h: ..., seed, offset, rng_state follow each other
DRAWS = {"zs_normal_sample_logprob": (2, 3, "fwd", 1), "zs_normal_sample_logprob_pair": (None, 2, "fwd", 2),
         "zs_normal_sample_logprob_bwd": (1, 2, "bwd", 1), "zs_logistic_sample_logprob": (2, 3, "fwd", 1),
         "zs_logistic_sample_logprob_bwd": (1, 2, "bwd", 1), "zs_uniform_sample": (4, 5, "fwd", 1),
         "zs_bernoulli_sample": (None, 4, "fwd", 1), "zs_philox_normal": (None, 2, "fwd", 1), "zs_philox_uniform": (None, 2, "fwd", 1)}
MULTI = {"zs_normal_sample_logprob_multi": "fwd", "zs_normal_sample_logprob_multi_bwd": "bwd"}


class Recorder(object):
    def __init__(self):
        self.launches = []           # dicts: entry, way ('fwd' / 'bwd'), ids [(seed, call), ...], step
        self.handed = []             # (step, seed, call) of every _rng.next_call, resolved
        self.step = 0
        self.inside_binding = False
        self._states = {}            # data_ptr -> rng_state tensor (kept alive, so that no address is reused)

    def know(self, t):
        if t is not None:
            self._states[t.data_ptr()] = t
        return t

    def resolve(self, seed, call, rs):
        """(seed, call) as the kernel forms them: {seed, base} of a state in memory replace the seed and add to the call."""
        if rs is not None and not isinstance(rs, torch.Tensor):
            rs = self._states[rs]                                   # KeyError: a state this test has not seen
        if rs is not None:
            s, base = rs.tolist()
            seed, call = s & M64, (base + call) & M64
        return int(seed) & M64, int(call) & M64

    def add(self, entry, way, ids):
        self.launches.append(dict(entry=entry, way=way, ids=ids, step=self.step))

    def forward_ids(self, step=None):
        return [i for l in self.launches if l["way"] == "fwd" and step in (None, l["step"]) for i in l["ids"]]

    # -- the main library
    def lib_call(self, name, args):
        base = name[:-4]
        if base in DRAWS:
            absent, at, way, n = DRAWS[base]
            if absent is None or args[absent] is None:
                s, c = self.resolve(args[at], args[at + 1], args[at + 2])
                self.add(base, way, [(s, (c + j) & M64) for j in range(n)])
        elif base in MULTI:
            terms, nt, seed, rs = args[0]._obj, args[1], args[2], args[3]
            ids = [self.resolve(seed, terms[t].offset, rs) for t in range(nt) if not terms[t].eps]
            if ids:
                self.add(base, MULTI[base], ids)

    # -- the samplers' bindings
    def mcmc_update(self, kind, kw):
        from zhusuan import _mcmc_hip
        z = kw.get("z")
        draws = kind != _mcmc_hip.SGHMC_PRE or bool(kw.get("flags", 0) & _mcmc_hip.RESAMPLE_V)
        if draws and (z is None or any(t is None for t in z)):
            self.add("zs_mcmc_update", "fwd", [self.resolve(kw.get("seed", 0), kw.get("call", 0), kw.get("rng_state"))])

    def hmc_move(self, kind, kw):
        from zhusuan import _hmc_hip
        z = kw.get("z")
        if kind == _hmc_hip.BEGIN and (z is None or any(t is None for t in z)):
            self.add("zs_hmc_move", "fwd", [self.resolve(kw.get("seed", 0), kw.get("call", 0), kw.get("rng_state"))])

    def hmc_decide(self, u, kw):
        if u is None:
            self.add("zs_hmc_decide", "fwd", [self.resolve(kw.get("seed", 0), kw.get("call", 0), kw.get("rng_state"))])


@contextlib.contextmanager
def recording():
    from zhusuan import _mcmc_hip, _hmc_hip
    rec = Recorder()
    klib = _hip.lib()
    saved = (klib.call, _ops._rng_snapshot, _rng.next_call, _mcmc_hip.update, _hmc_hip.move, _hmc_hip.decide)

    def call(name, *a):
        if not rec.inside_binding:         # (the host restatement of a sampler binding fetches its launch's stream from the oracle)
            rec.lib_call(name, a)
        return saved[0](name, *a)

    def bound(i, *a, **k):
        rec.inside_binding = True
        try:
            return saved[i](*a, **k)
        finally:
            rec.inside_binding = False

    def snapshot(*a, **k):
        return rec.know(saved[1](*a, **k))

    def next_call(device):
        s, c, rs = saved[2](device)
        rec.handed.append((rec.step,) + rec.resolve(s, c, rec.know(rs)))
        return s, c, rs

    def update(kind, *a, **k):
        rec.mcmc_update(kind, k)
        return bound(3, kind, *a, **k)

    def move(kind, *a, **k):
        rec.hmc_move(kind, k)
        return bound(4, kind, *a, **k)

    def decide(chunks, n_chains, logp0, logp1, u, *a, **k):
        rec.hmc_decide(u, k)
        return bound(5, chunks, n_chains, logp0, logp1, u, *a, **k)
    klib.call, _ops._rng_snapshot, _rng.next_call, _mcmc_hip.update, _hmc_hip.move, _hmc_hip.decide = \
        call, snapshot, next_call, update, move, decide
    try:
        yield rec
    finally:
        klib.call, _ops._rng_snapshot, _rng.next_call, _mcmc_hip.update, _hmc_hip.move, _hmc_hip.decide = saved


# ------------------------------------------------------------------------------------------------ the two id sources
def _generator_position(dev):
    """(seed, number of call ids handed out so far) of the generator path (_rng._seed_and_call: off // 4)."""
    if dev.type == "cpu":
        return host_backend._state["seed"] & M64, host_backend._state["call"]
    gen = torch.cuda.default_generators[dev.index or 0]
    assert gen.get_offset() % 4 == 0
    return gen.initial_seed() & M64, gen.get_offset() // 4


def _seed(dev):
    torch.manual_seed(SEED)
    if dev.type == "cpu":
        host_backend.manual_seed(SEED)


def run_generator(dev, make_step):
    step = make_step()                       # (building a model may seed torch itself: seed afterwards)
    _seed(dev)
    with recording() as rec:
        seed, start = _generator_position(dev)
        assert seed == SEED
        for s in range(STEPS):
            rec.step = s
            step()
        _, end = _generator_position(dev)
    # off // 4, and every draw advances the offset by 4: the k-th id handed out is start + k, whatever was launched with it
    assert [h[1:] for h in rec.handed] == [(SEED, start + k) for k in range(end - start)]
    return rec


def run_device_rng(dev, make_step, stride=1 << 16):
    step = make_step()
    _seed(dev)
    rng = zs.DeviceRNG(dev, seed=2 ** 64 - 1 - 12345, stride=stride)      # bit 63 set: the state keeps the lower 63 bits
    want_seed = (2 ** 64 - 1 - 12345) & (2 ** 63 - 1)
    with recording() as rec, zs.device_rng(rng):
        rec.know(rng.state)
        before = _generator_position(dev)
        for s in range(STEPS):
            rec.step = s
            rng.begin_step()
            step()
        assert _generator_position(dev) == before, "a draw went to the generator although a DeviceRNG is set"
    # base + delta: delta restarts at 0 in every step, base moves by stride
    for s in range(STEPS):
        mine = [h[1:] for h in rec.handed if h[0] == s]
        assert mine == [(want_seed, (s + 1) * stride + d) for d in range(len(mine))], s
    assert rng.state.tolist() == [want_seed, STEPS * stride]
    return rec


def check(rec, expect_entries=()):
    fwd = rec.forward_ids()
    assert fwd, "the scenario drew nothing through the recorded layer"
    dup = sorted({i for i in fwd if fwd.count(i) > 1})
    assert not dup, "(seed, call id) used by two forward draws: %s" % [
        (l["entry"], l["step"]) for l in rec.launches if l["way"] == "fwd" and set(l["ids"]) & set(dup)]
    handed = {h[1:] for h in rec.handed}
    for l in rec.launches:
        if l["entry"] == "zs_normal_sample_logprob_pair":
            (s0, c0), (s1, c1) = l["ids"]
            assert s0 == s1 and c1 == c0 + 1, l
        if l["way"] == "fwd":
            assert set(l["ids"]) <= handed, ("an id that _rng.next_call never handed out", l)
        else:
            assert set(l["ids"]) <= set(rec.forward_ids(l["step"])), ("a backward regenerates a draw its step never made", l)
    names = {l["entry"] for l in rec.launches}
    for e in expect_entries:
        assert e in names, (e, sorted(names))
    return rec


RUNNERS = [pytest.param(run_generator, id="generator"), pytest.param(run_device_rng, id="device_rng")]


# ------------------------------------------------------------------------------------------------ the callers
def _train_step(model, obs):
    def step():
        model.zero_grad()
        model(obs).backward()
    return step


def vae(dev):
    from examples import vae_mnist
    model = vae_mnist.build(4, hidden=16, device=dev)
    return _train_step(model, {"x": torch.tensor(H.vae_data(4)[0], device=dev)})


def iwae_vimco(dev):
    from examples import iwae
    model = iwae.build(n_samples=3, estimator="vimco", hidden=16, device=dev)
    return _train_step(model, {"x": torch.tensor(H.iwae_data(4, 3)[0], device=dev)})


def hierarchical(dev):
    """A two-latent variational net whose second latent is computed from the first (tests/test_one_launch.py)."""
    class Q(BayesianNet):
        def __init__(self):
            super().__init__()
            self.mu = torch.nn.Parameter(torch.zeros(6, 8))

        def forward(self, observed):
            self.observe(observed)
            one = torch.ones_like(self.mu.detach())
            z1 = self.normal("z1", mean=self.mu, std=one, reduce_mean_dims=[0], reduce_sum_dims=[1])
            self.normal("z2", mean=torch.tanh(z1) * 0.5, std=one, reduce_mean_dims=[0], reduce_sum_dims=[1])
            return self

    class P(BayesianNet):
        def __init__(self):
            super().__init__()
            self.s = torch.nn.Parameter(torch.ones(1))

        def forward(self, observed):
            self.observe(observed)
            one = torch.ones(6, 8, device=self.s.device)
            z1 = self.normal("z1", mean=0 * one, std=one, reduce_mean_dims=[0], reduce_sum_dims=[1])
            z2 = self.normal("z2", mean=z1 * self.s, std=one, reduce_mean_dims=[0], reduce_sum_dims=[1])
            self.normal("x", mean=z2, std=one, reduce_mean_dims=[0], reduce_sum_dims=[1])
            return self
    model = ELBO(P(), Q()).to(dev)
    return _train_step(model, {"x": torch.zeros(6, 8, device=dev)})


def bnn(dev):
    from examples import bnn_vi
    model = bnn_vi.build(n_particles=4, device=dev)
    x, y, _ = H.bnn_data(8, 4)
    return _train_step(model, {"x": torch.tensor(x, device=dev), "y": torch.tensor(y, device=dev)})


def flow_vae(dev):
    import test_flow_elbo as FE
    model = FE.build("NICE", dev)
    return _train_step(model, {"x": FE.data(dev)[0]})


def sgmcmc(name):
    def make(dev):
        import test_mcmc_samplers as MS
        net = MS.independent_normals(dev, 40)
        sampler = dict(MS.samplers())[name]()
        first = [True]

        def step():
            if first[0]:                      # the chains' starting points: two prior draws per latent
                sampler.sample(net, {}, resample=True)
                first[0] = False
            sampler.sample(net, {})
        return step
    return make


def hmc(dev):
    import test_hmc_sampler as HS
    from zhusuan.mcmc import HMC
    C = 3
    x, y = HS.blr_data(C)
    net = HS.blr_net(dev, C)
    obs = {'x': x.to(dev), 'y': y.to(dev)}
    latent = [{'w': torch.zeros(C, 5, device=dev), 'b': torch.zeros(C, 2, 3, device=dev)}]
    h = HMC(step_size=0.05, n_leapfrogs=2)

    def step():
        for _ in range(2):
            latent[0], _info = h.sample(net, obs, latent[0])
    return step


CALLERS = [
    ("vae", vae, True, ["zs_normal_sample_logprob_pair", "zs_normal_sample_logprob_bwd"]),
    ("iwae_vimco_paired", iwae_vimco, True, ["zs_normal_sample_logprob_pair"]),
    ("iwae_vimco_unpaired", iwae_vimco, False, ["zs_normal_sample_logprob"]),
    ("hierarchical", hierarchical, True, ["zs_normal_sample_logprob_pair", "zs_normal_sample_logprob_bwd"]),
    ("bnn_ms1", bnn, True, ["zs_normal_sample_logprob", "zs_normal_sample_logprob_multi", "zs_normal_sample_logprob_multi_bwd"]),
    ("flow_vae", flow_vae, True, ["zs_normal_sample_logprob", "zs_normal_sample_logprob_bwd"]),      # (z of 5: no pair launch)
    ("sgld", sgmcmc("sgld"), True, ["zs_normal_sample_logprob", "zs_mcmc_update"]),
    ("psgld", sgmcmc("psgld"), True, ["zs_mcmc_update"]),
    ("sghmc_first_order", sgmcmc("sghmc1"), True, ["zs_mcmc_update"]),
    ("sghmc_second_order", sgmcmc("sghmc2"), True, ["zs_mcmc_update"]),
    ("hmc", hmc, True, ["zs_hmc_move", "zs_hmc_decide"]),
]


@pytest.mark.parametrize("runner", RUNNERS)
@pytest.mark.parametrize("name,make,paired,entries", CALLERS, ids=[c[0] for c in CALLERS])
def test_no_id_is_handed_to_two_draws(adev, runner, name, make, paired, entries):
    with zs.pair_draws(paired):
        rec = check(runner(adev, lambda: make(adev)), entries)
    if name == "iwae_vimco_unpaired":
        assert not any(l["entry"] == "zs_normal_sample_logprob_pair" for l in rec.launches)
    if name.startswith(("sg", "psg")):
        # 40 latents run as two chunks (32 + 8): every drawing update of a step has its own id
        per_step = [[l for l in rec.launches if l["entry"] == "zs_mcmc_update" and l["step"] == s] for s in range(STEPS)]
        assert all(len(p) >= 2 and len(p) % 2 == 0 for p in per_step), [len(p) for p in per_step]
    if name == "hmc":
        assert [l["entry"] for l in rec.launches] == ["zs_hmc_move", "zs_hmc_decide"] * (2 * STEPS)


@pytest.fixture
def host_dev():
    with host_routing.host(*ROUTERS) as dev:
        yield dev


def test_the_check_notices_an_id_handed_out_twice(host_dev, monkeypatch):
    """The point of this file, turned round: an id source that hands every second draw the id of the one before it (two
    latents drawing the same noise) must not pass.  The sabotage is applied to the host back-end's id source."""
    adev = host_dev
    inner = _rng._seed_and_call
    last = []

    def stuck(device):
        s, c = inner(device)
        if c % 2 == 1 and last:
            return last[0]
        last[:] = [(s, c)]
        return s, c
    caught = []
    for make, paired in ((hierarchical, True), (bnn, True), (sgmcmc("sgld"), True)):
        with monkeypatch.context() as m:
            m.setattr(_rng, "_seed_and_call", stuck)
            host_backend.manual_seed(SEED)
            step = make(adev)
            with zs.pair_draws(paired), recording() as rec:
                try:
                    step()
                except RuntimeError as e:          # the pair draw's own guard: "not consecutive"
                    assert "consecutive" in str(e)
                    caught.append("guard")
                    continue
            with pytest.raises(AssertionError, match="used by two forward draws"):
                check(rec)
            caught.append("check")
    assert caught.count("check") >= 2, caught


# ------------------------------------------------------------------------------------------------ without the hook
@contextlib.contextmanager
def sampled_normals():
    """Every tensor a Normal node returns from a draw, with the node's parameters: collected at the distribution, a layer
    above the recorder's."""
    from zhusuan.distributions.normal import Normal
    inner, seen = Normal._sample, []

    def _sample(self, *a, **k):
        z = inner(self, *a, **k)
        seen.append((z, self))
        return z
    Normal._sample = _sample
    try:
        yield seen
    finally:
        Normal._sample = inner


def _standardised(z, dist, n=64):
    mean, scale = dist._mean.detach().double(), dist._scale_operand().detach().double()
    std = torch.exp(scale) if dist._logstd_given is not None else scale
    e = (z.detach().double() - mean) / std
    assert e.numel() >= n
    return e.reshape(-1)[:n].cpu().numpy()


@pytest.mark.parametrize("name,make,nodes", [("iwae", iwae_vimco, 1), ("bnn", bnn, 2)])
def test_no_two_draws_of_a_step_are_the_same_noise(adev, name, make, nodes):
    """One step under the seeded generator: both draws of every latent (the factory's and the objective's re-read, which
    ends up in the node's sample_cache), standardised; no two agree on their first 64 elements."""
    model_step = make(adev)
    _seed(adev)
    with sampled_normals() as seen:
        model_step()
    dists = []
    for _, d in seen:
        if not any(d is e for e in dists):
            dists.append(d)
    draws = [(z, d) for z, d in seen] + [(d.sample_cache, d) for d in dists]
    uniq = []
    for z, d in draws:
        if not any(z is u[0] or (z.data_ptr() == u[0].data_ptr() and z.shape == u[0].shape) for u in uniq):
            uniq.append((z, d))
    assert len(dists) == nodes and len(uniq) == 2 * nodes, (len(dists), len(uniq))
    eps = [_standardised(z, d) for z, d in uniq]
    for i in range(len(eps)):
        assert np.isfinite(eps[i]).all() and np.abs(eps[i]).max() < 7.0
        for j in range(i):
            assert not (np.abs(eps[i] - eps[j]) <= 1e-6).all(), "draws %d and %d are the same noise" % (j, i)
