"""``zhusuan.mcmc`` at the level of its public interface, on both back-ends of the suite's ``dev`` fixture: "hip" is the
package on libzs_mcmc.so, "host" the same package code with the update function of the binding replaced by the torch
restatement of tests/mcmc_host.py (and the other kernels by the C oracle, tests/host_backend.py)."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import host_backend
import mcmc_models as M
from conftest import PKG_ROOT
import truth
from mcmc_host import mdev  # noqa: F401
from truth import seed_all


def bnn(dev, layers=(3, 4, 1)):
    from zhusuan.framework.bn import BayesianNet
    x, y = M.make_data(3, layers[0])
    return M.make_net(BayesianNet, list(layers), device=dev), {'x': torch.tensor(x, device=dev), 'y': torch.tensor(y, device=dev)}


def independent_normals(dev, k, dtype=torch.float32, mean=0.5, std=2.0):
    """k latent nodes z0 .. z{k-1} of 1 to 5 elements, N(mean, std^2) each: the gradient of the log joint is -(z - mean) / std^2."""
    from zhusuan.framework.bn import BayesianNet

    class Net(BayesianNet):
        def forward(self, observed):
            self.observe(observed)
            for i in range(k):
                n = 1 + i % 5
                self.normal('z%d' % i, mean=torch.full([n], mean, dtype=dtype, device=dev),
                            std=torch.full([n], std, dtype=dtype, device=dev), group_ndims=1)
            return self
    return Net().to(dev)


def samplers():
    from zhusuan.mcmc import SGLD, PSGLD, SGHMC
    return [("sgld", lambda: SGLD(1e-3)), ("psgld", lambda: PSGLD(1e-3)),
            ("sghmc1", lambda: SGHMC(1e-3, friction=0.3, variance_estimate=0.02, n_iter_resample_v=2, second_order=False)),
            ("sghmc2", lambda: SGHMC(1e-3, friction=0.3, variance_estimate=0.02, n_iter_resample_v=2, second_order=True))]


class Counted(object):
    """Wraps the binding's single update function (whichever is installed) and records every launch."""

    def __enter__(self):
        from zhusuan import _mcmc_hip
        self.mod, self.inner, self.launches = _mcmc_hip, _mcmc_hip.update, []

        def update(kind, q_in, *args, **kw):
            self.launches.append((kind, len(q_in), q_in[0].dtype))
            return self.inner(kind, q_in, *args, **kw)
        _mcmc_hip.update = update
        return self

    def __exit__(self, *exc):
        self.mod.update = self.inner


# ------------------------------------------------------------------------------------------------ interface
def test_import_forms_and_constructor_defaults():
    import zhusuan as zs
    import zhusuan.mcmc
    from zhusuan.mcmc import SGLD, PSGLD, SGHMC
    from zhusuan.mcmc.SGLD import SGLD as SGLD2, PSGLD as PSGLD2
    from zhusuan.mcmc.SGHMC import SGHMC as SGHMC2
    from zhusuan.mcmc.SGMCMC import SGMCMC
    assert SGLD is SGLD2 and PSGLD is PSGLD2 and SGHMC is SGHMC2 and zs.mcmc.SGLD is SGLD
    assert issubclass(PSGLD, SGLD) and issubclass(SGLD, SGMCMC) and issubclass(SGHMC, SGMCMC)
    s = zs.mcmc.SGLD(learning_rate=1e-3)
    assert s.t == 0 and math.isclose(s.lr, 1e-3) and s.device == torch.device('cpu')
    p = PSGLD(1e-3)
    assert (p.decay, p.epsilon) == (0.9, 1e-3) and p.aux is None
    h = SGHMC(1e-3)
    assert (h.alpha, h.beta, h.n_iter_resample_v, h.second_order) == (0.25, 0., 20, True) and h.vs is None
    assert SGHMC(1e-3, n_iter_resample_v=None).n_iter_resample_v == 0
    s.t = 5
    s.initialize()
    assert s.t == 0
    assert s.to(torch.device('cpu')) is s


def test_import_zhusuan_does_not_load_the_sampler_binding():
    code = ("import sys; sys.path.insert(0, %r)\nimport zhusuan\n"
            "assert 'zhusuan.mcmc' not in sys.modules and 'zhusuan._mcmc_hip' not in sys.modules\n"
            "import zhusuan.mcmc\nfrom zhusuan import _mcmc_hip\nassert _mcmc_hip._LIB is None\nprint('LAZY')\n") % PKG_ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert "LAZY" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("name", ["sgld", "psgld", "sghmc1", "sghmc2"])
def test_resample_step_and_aliasing(mdev, name):
    make = dict(samplers())[name]
    net, obs = bnn(mdev)
    seed_all(4, mdev)
    a = make()
    first = a.sample(net, obs, resample=True)
    assert a.t == 1 and list(first.keys()) == ['w0', 'w1'] and a.device == mdev
    assert tuple(first['w0'].shape) == (3, 4, 4) and tuple(first['w1'].shape) == (3, 1, 5)
    for q, k in zip(a._var_list, first):
        assert q.is_leaf and q.requires_grad and q.grad_fn is None and torch.equal(q.detach(), first[k].detach())
    kept = dict((k, v.detach().clone()) for k, v in first.items())
    out3 = a.sample(net, obs, step=3)
    assert a.t == 4
    for k in first:                                    # new tensors every step: what the caller kept is unchanged
        assert torch.equal(first[k].detach(), kept[k]) and out3[k].data_ptr() != first[k].data_ptr()
        assert out3[k].is_leaf and out3[k].requires_grad and bool(torch.isfinite(out3[k]).all())
        assert not torch.equal(out3[k].detach(), kept[k])
    seed_all(4, mdev)
    b = make()
    again = b.sample(net, obs, resample=True)
    outs = [b.sample(net, obs) for _ in range(3)]
    assert b.t == 4
    for k in first:
        assert torch.equal(again[k].detach(), kept[k])
        assert torch.equal(outs[2][k].detach(), out3[k].detach()), "step=3 differs from three single calls"
        assert len(set(o[k].data_ptr() for o in outs)) == 3
        assert not torch.equal(outs[0][k].detach(), outs[1][k].detach())


def test_an_observed_latent_is_not_updated(mdev):
    from zhusuan.mcmc import SGLD
    net, obs = bnn(mdev)
    w1 = torch.full((3, 1, 5), 0.25, device=mdev)
    obs = dict(obs, w1=w1)
    s = SGLD(1e-3)
    seed_all(1, mdev)
    first = s.sample(net, obs, resample=True)
    assert list(first.keys()) == ['w0']
    with Counted() as c:
        out = s.sample(net, obs, step=2)
    assert list(out.keys()) == ['w0'] and [l[1] for l in c.launches] == [1, 1]
    assert bool((w1 == 0.25).all())


@pytest.mark.parametrize("name", ["sgld", "psgld", "sghmc1", "sghmc2"])
def test_launches_per_step(mdev, name):
    from zhusuan import _mcmc_hip
    make = dict(samplers())[name]
    net, obs = bnn(mdev)
    s = make()
    seed_all(2, mdev)
    s.sample(net, obs, resample=True)
    for t in range(1, 5):
        with Counted() as c:
            s.sample(net, obs)
        assert all(l[1] == 2 for l in c.launches), c.launches              # both latents in every launch
        kinds = [l[0] for l in c.launches]
        if name == "sgld":
            assert kinds == [_mcmc_hip.SGLD]
        elif name == "psgld":
            assert kinds == [_mcmc_hip.PSGLD]
        elif name == "sghmc2":
            assert kinds == [_mcmc_hip.SGHMC_PRE, _mcmc_hip.SGHMC_POST]
        else:       # first order: a launch before the gradient only when velocities are drawn (first update, t % 2 == 0)
            assert kinds == ([_mcmc_hip.SGHMC_PRE] if (t == 1 or t % 2 == 0) else []) + [_mcmc_hip.SGHMC_POST]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_forty_latents_split_across_two_launches(mdev, dtype):
    """SGLD on 40 independent Normal latents with injected noise: q' = q + (lr/2) g + sqrt(lr) z with g = -(q - mean) / std^2,
    held to the float64 evaluation within 2^-20 (2^-48 for float64) of the sum of the terms' magnitudes, as the kernel tests."""
    import zhusuan
    from zhusuan.mcmc import SGLD
    k, lr = 40, 1e-2
    net = independent_normals(mdev, k, dtype)
    gen = truth.gen(8)
    shapes = [(1 + i % 5,) for i in range(k)]
    prior = [torch.randn(s, generator=gen, dtype=torch.float64).to(dtype) for s in shapes * 2]
    noise = [torch.randn(s, generator=gen, dtype=torch.float64).to(dtype) for s in shapes]
    s = SGLD(lr)
    with zhusuan.inject_epsilon(prior + noise):
        first = s.sample(net, {}, resample=True)
        with Counted() as c:
            out = s.sample(net, {})
    assert [l[1:] for l in c.launches] == [(32, dtype), (8, dtype)]
    assert list(out.keys()) == ['z%d' % i for i in range(k)]
    rel = 2.0 ** -20 if dtype == torch.float32 else 2.0 ** -48
    for i in range(k):
        q = first['z%d' % i].detach().cpu().double()
        assert torch.equal(q, (0.5 + 2.0 * prior[k + i].double()).to(dtype).double())       # the sampler's re-read of node.tensor
        terms = [q, 0.5 * lr * (-(q - 0.5) / 4.0), math.sqrt(lr) * noise[i].double()]
        got = out['z%d' % i].detach().cpu()
        assert got.dtype == dtype
        err = (got.double() - sum(terms)).abs()
        assert bool((err <= rel * sum(t.abs() for t in terms)).all()), (i, float(err.max()))


def test_example_runs_three_steps(mdev):
    from examples import bnn_sgmcmc
    for name in ("sgld", "sghmc"):
        seed_all(0, mdev)
        rmse = bnn_sgmcmc.run(steps=3, batch=8, particles=2, layer_sizes=(3, 4, 1), sampler=name, device=mdev, n_train=16, n_test=8)
        assert isinstance(rmse, float) and math.isfinite(rmse) and rmse > 0


# ------------------------------------------------------------------------------------------------ gpu only
def _trajectory(dev, make, steps=3):
    net, obs = bnn(dev)
    s = make()
    out = [s.sample(net, obs, resample=True)]
    out += [s.sample(net, obs) for _ in range(steps)]
    return [torch.cat([o[k].detach().flatten() for k in o]).cpu() for o in out]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sgld", "sghmc2"])
def test_cuda_manual_seed_reproduces_a_run(name):
    dev = torch.device("cuda:0")
    host_backend.uninstall()
    make = dict(samplers())[name]
    torch.cuda.manual_seed(21)
    a = _trajectory(dev, make)
    torch.cuda.manual_seed(21)
    b = _trajectory(dev, make)
    torch.cuda.manual_seed(22)
    c = _trajectory(dev, make)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert all(not torch.equal(x, y) for x, y in zip(a, c))


@pytest.mark.gpu
def test_device_rng_routes_the_update_through_its_state():
    """One SGLD update under ``zhusuan.device_rng(DeviceRNG(dev, seed))`` equals the same update with the noise handed in
    explicitly: flat elements of zs_philox_normal_f32(seed, call = the rng's base + delta) in latent order."""
    import zhusuan
    from zhusuan import _hip
    from zhusuan.mcmc import SGLD
    dev = torch.device("cuda:0")
    host_backend.uninstall()
    net, obs = bnn(dev)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mcmc", "g_mcmc_sgld.npz"))
    prior = [g["draw_%02d" % i] for i in range(4)]
    seed, n = 1234, 48 + 15

    def start():
        s = SGLD(1e-3)
        with zhusuan.inject_epsilon(prior):
            s.sample(net, obs, resample=True)
        return s
    rng = zhusuan.DeviceRNG(dev, seed=seed)
    rng.begin_step()                                   # base = one stride
    a = start()
    with zhusuan.device_rng(rng):
        out_a = a.sample(net, obs)
    z = torch.empty(n, device=dev)
    _hip.lib().call("zs_philox_normal_f32", z.data_ptr(), n, seed, rng.stride, None, _hip.stream_for(z))
    b = start()
    with zhusuan.inject_epsilon([z[:48].view(3, 4, 4), z[48:].view(3, 1, 5)]):
        out_b = b.sample(net, obs)
    for k in out_a:
        assert torch.equal(out_a[k].detach(), out_b[k].detach())
    with zhusuan.device_rng(rng):                      # the next draw of the step uses the next delta: other noise
        out_c = start().sample(net, obs)
    assert not torch.equal(out_c['w0'].detach(), out_a['w0'].detach())


@pytest.mark.gpu
def test_missing_library_names_the_build_command_and_leaves_the_rest_working(tmp_path, monkeypatch):
    from zhusuan import _mcmc_hip
    from zhusuan.mcmc import SGLD
    from examples import bnn_vi
    dev = torch.device("cuda:0")
    host_backend.uninstall()
    missing = str(tmp_path / "libzs_mcmc.so")
    with pytest.raises(RuntimeError, match="make -C zhusuan-pytorch_amd/csrc mcmc"):
        _mcmc_hip.lib(missing)
    # a sampler whose binding finds no library: the prior draws work (main library), the update raises, nothing falls back
    monkeypatch.setattr(_mcmc_hip, "LIB_PATH", missing)
    monkeypatch.setattr(_mcmc_hip, "_LIB", None)
    net, obs = bnn(dev)
    s = SGLD(1e-3)
    first = s.sample(net, obs, resample=True)
    with pytest.raises(RuntimeError, match="make -C zhusuan-pytorch_amd/csrc mcmc"):
        s.sample(net, obs)
    assert bool(torch.isfinite(first['w0']).all())
    model = bnn_vi.build(layer_sizes=(3, 4, 1), n_particles=2, multiplier=6, device=dev)
    loss = model(obs)
    loss.backward()
    assert math.isfinite(float(loss))
