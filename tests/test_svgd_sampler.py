"""zhusuan.mcmc.SVGD: the public interface on the CPU (the torch composition) and on the GPU (the three kernels of
libzs_svgd.so).  See tests/README_svgd.md.

The net is a two-latent Gaussian, log p = -(w - 1)^2 / (2 * 0.49) - b^2 / 8 summed over an event, so SVGD is a deterministic map
and whole trajectories are compared with the float64 truth of tests/test_svgd_kernel.py iterated from the same start.  Tolerance of
an N-step trajectory: a step adds at most STEP B + 2 u max|q| (B: the bound of phi of test_svgd_kernel.bounds at the start, u the
unit of the coarsest latent) and earlier errors grow by at most 1 + STEP L a step, L <= 1 / 0.49 + 2 / h the Lipschitz constant of
phi near the cloud (h > 1 for these clouds): with STEP = 0.01, 1.05^20 < 4, hence 4 N (STEP B + 2 u max|q|)."""
import subprocess
import sys

import pytest
import torch

import host_routing
from kernel_abi import F32, F64, unit
from test_svgd_kernel import bounds, close, truth

import zhusuan as zs
from zhusuan.framework.bn import BayesianNet
from zhusuan.mcmc import SVGD, SVGDInfo

STEP = 0.01
CALLS = host_routing.Router("zhusuan._svgd_hip", dict.fromkeys(["gram", "finish", "update"]))


class Net(BayesianNet):
    def forward(self, observed):
        self.observe(observed)
        return self

    def _log_joint(self):
        w, b = self.observed['w'], self.observed['b']
        return (-(w - 1) ** 2 / 0.98).sum(-1).to(b.dtype) - (b ** 2 / 8).sum((-1, -2))


def start(shape, dtypes, dev="cpu"):
    gen = torch.Generator().manual_seed(7 + len(shape))
    w, b = torch.randn(*shape, 5, generator=gen), torch.randn(*shape, 2, 3, generator=gen)
    return {'w': w.to(dev, dtypes[0]), 'b': b.to(dev, dtypes[1])}


def true_steps(latent, n, K):
    """n steps of the float64 truth; (trajectory end as [K, M] tensors, the last step's (phis, kernel, h), its start)"""
    q = [latent['w'].cpu().double().reshape(K, -1), latent['b'].cpu().double().reshape(K, -1)]
    for _ in range(n):
        before = q
        t = truth(q, [-(q[0] - 1) / 0.49, -q[1] / 4])
        q = [a + STEP * p for a, p in zip(q, t[0])]
    return q, t, before


def check_run(latent, n, K, dtypes, inplace=False):
    svgd = SVGD(step_size=STEP)
    net = Net().to(latent['w'].device)
    first = [latent['w'].cpu().double().reshape(K, -1), latent['b'].cpu().double().reshape(K, -1)]
    coarse = F32 if F32 in dtypes else F64
    B = bounds(coarse, first, [-(first[0] - 1) / 0.49, -first[1] / 4], truth(first, [-(first[0] - 1) / 0.49, -first[1] / 4]))[0]
    cur = latent
    for _ in range(n):
        given = cur
        cur, info = svgd.sample(net, {}, cur, inplace=inplace)
        assert (cur['w'] is given['w']) == inplace and isinstance(info, SVGDInfo)
    want, t, before = true_steps(latent if not inplace else {k: v0 for k, v0 in zip(('w', 'b'), first)}, n, K)
    for got, w in zip((cur['w'], cur['b']), want):
        assert got.shape == latent['w'].shape[:-1] + got.shape[len(latent['w'].shape) - 1:]
        close("trajectory", got.reshape(K, -1), w, 4 * n * (STEP * B + 2 * unit(coarse) * float(w.abs().max())))
    return svgd, info, t, before


def test_exports_and_lazy_loading():
    assert "SVGD" in zs.mcmc.__all__ if hasattr(zs.mcmc, "__all__") else hasattr(zs.mcmc, "SVGD")
    code = "import sys, zhusuan; assert 'zhusuan._svgd_hip' not in sys.modules and 'zhusuan.mcmc' not in sys.modules"
    assert subprocess.run([sys.executable, "-c", code], env=dict(__import__("os").environ, PYTHONPATH=":".join(sys.path))).returncode == 0


def test_argument_errors():
    for kw in (dict(step_size=0), dict(bandwidth=0.0), dict(bandwidth=-1), dict(alpha=1.0), dict(fudge=0)):
        with pytest.raises(ValueError):
            SVGD(**kw)
    svgd, net = SVGD(), Net()
    good = start((7,), (F64, F64))
    with pytest.raises(ValueError, match="no latent"):
        svgd.sample(net, {}, {})
    with pytest.raises(ValueError, match="float32 or float64"):
        svgd.sample(net, {}, dict(good, w=good['w'].half()))
    with pytest.raises(ValueError, match="not contiguous"):
        svgd.sample(net, {}, dict(good, b=good['b'].transpose(1, 2)), inplace=True)
    with pytest.raises(ValueError, match="does not begin with the particle shape"):
        svgd.sample(net, {}, dict(good, w=good['w'][:1]))          # (broadcasts in the net)


@pytest.mark.parametrize("n", [1, 5])
def test_torch_path_on_the_cpu(n):
    svgd, info, t, _ = check_run(start((7,), (F64, F64)), n, 7, (F64, F64))
    assert svgd.last_path["path"].startswith("torch composition") and "CPU" in svgd.last_path["why"] and svgd.t == n
    close("kernel", info.kernel, t[1], 1e-12)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dtypes,inplace", [((7,), (F32, F32), False), ((32,), (F64, F64), False), ((7,), (F32, F64), False),
                                                  ((32,), (F32, F32), True), ((4, 8), (F32, F64), False)])
def test_twenty_steps_on_the_gpu(shape, dtypes, inplace):
    K = int(torch.Size(shape).numel())
    latent = start(shape, dtypes, "cuda:0")
    with CALLS.recording() as calls:
        svgd, info, t, before = check_run(latent, 20, K, dtypes, inplace)
    chunks = len(set(dtypes))
    assert [c.name for c in calls] == (["gram"] * chunks + ["finish"] + ["update"] * chunks) * 20
    assert svgd.last_path["why"] is None and svgd.last_path["path"].startswith("S1-S3 zs_svgd_gram") and svgd.t == 20
    coarse = F32 if F32 in dtypes else F64
    _, bk, bh = bounds(coarse, before, [-(before[0] - 1) / 0.49, -before[1] / 4], t)
    # the last step's info, at a start that differs from the truth's by the trajectory's tolerance: d moves by 2 sqrt(d) times that
    slack = 1e-3 if coarse == F32 else 1e-11
    close("info.kernel", info.kernel, t[1], bk + slack)
    close("info.bandwidth", info.bandwidth, torch.tensor(t[2], dtype=F64), bh + slack * t[2])
    lp = -((before[0] - 1) ** 2 / 0.98).sum(1) - (before[1] ** 2 / 8).sum(1)
    assert info.log_prob.shape == shape and info.kernel.shape == (K, K) and info.bandwidth.shape == ()
    close("info.log_prob", info.log_prob.reshape(K), lp, 64 * unit(coarse) * (1 + lp.abs()) + slack * (1 + lp.abs()))


@pytest.mark.gpu
def test_wide_particle_set_takes_the_torch_path():
    latent = start((300,), (F32, F32), "cuda:0")
    with CALLS.recording() as calls:
        svgd, _, _, _ = check_run(latent, 1, 300, (F32, F32))
    assert calls == [] and svgd.last_path["path"].startswith("torch composition") and "300" in svgd.last_path["why"]
