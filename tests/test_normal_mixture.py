"""NormalMixture and ``BayesianNet.normal_mixture`` (zhusuan/distributions/mixture.py): the public interface over the kernels of
include/zs_mix.h.  The truth and the bounds are those of tests/test_mix_kernel.py."""
import os
import subprocess
import sys

import pytest
import torch

import zhusuan as zs
from zhusuan.distributions import NormalMixture
from zhusuan.framework.bn import BayesianNet
from cat_host import cdev  # noqa: F401
from test_mix_kernel import NAMES, bounds, case_inputs, truth

F32, F64 = torch.float32, torch.float64
K, B, D, C = 3, 5, 5, 17


def test_import_loads_neither_the_binding_nor_the_library():
    code = ("import sys, zhusuan; assert 'zhusuan._mix_hip' not in sys.modules; "
            "from zhusuan.distributions import NormalMixture; assert 'zhusuan._mix_hip' not in sys.modules; "
            "from zhusuan import _mix_hip; assert _mix_hip._LIB is None")
    pkg_root = os.path.dirname(os.path.dirname(os.path.abspath(zs.__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=pkg_root, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


def test_construction_shapes_and_errors():
    lg, mu, sc = torch.zeros(4), torch.zeros(4, 7), torch.ones(4, 7)
    d = NormalMixture(lg, mu, std=sc, batch_shape=(3,), device="cpu")
    assert tuple(d.batch_shape) == (3,) and (d.n_components, d.n_dims) == (4, 7) and d.dtype == F32
    assert d.is_continuous and not d.is_reparameterized and torch.equal(d.logstd, torch.zeros(4, 7))
    for shape in ((7,), (3, 7), (2, 3, 7)):
        assert tuple(d.log_prob(torch.ones(shape)).shape) == shape[:-1]
    assert tuple(NormalMixture(lg, mu, logstd=sc, group_ndims=1, device="cpu").log_prob(torch.ones(2, 3, 7)).shape) == (2,)
    for kw in (dict(), dict(std=sc, logstd=sc)):
        with pytest.raises(ValueError, match="Either `std` or `logstd`"):
            NormalMixture(lg, mu, device="cpu", **kw)
    with pytest.raises(ValueError, match=r"\[C\].*\(4, 1\)"):
        NormalMixture(lg[:, None], mu, std=sc, device="cpu")
    with pytest.raises(ValueError, match=r"\[4, D\].*\(5, 7\)"):
        NormalMixture(lg, torch.zeros(5, 7), std=sc, device="cpu")
    with pytest.raises(ValueError, match=r"std .*\(4, 7\).*\(4, 6\)"):
        NormalMixture(lg, mu, std=torch.ones(4, 6), device="cpu")
    with pytest.raises(ValueError, match=r"7 entries.*\(3, 8\)"):
        d.log_prob(torch.ones(3, 8))


@pytest.mark.parametrize("n", [None, 4])
def test_shape_of_a_sample(cdev, n):
    d = NormalMixture(torch.zeros(6, device=cdev), torch.zeros(6, 3, device=cdev), logstd=torch.zeros(6, 3, device=cdev), batch_shape=(2, 5))
    z = d.sample(n)
    assert tuple(z.shape) == (() if n is None else (n,)) + (2, 5, 3) and not z.requires_grad and z.dtype == F32
    assert tuple(d.log_prob(z).shape) == tuple(z.shape[:-1])


def check_against_truth(device, dtype, D=D, via_bn=False, scale="logstd"):
    """log_prob / log_joint of a value [K, B, D] and autograd.grad for x, logits, mean and logstd against the float64 truth, within
    the kernel test's bounds for `dtype`; returns the mixture distribution."""
    ins = case_inputs(D, C, K * B)
    lg, mu, ls, x = (a.to(device, dtype).clone().requires_grad_(True) for a in ins[:4])
    g = ins[4]
    if via_bn:
        class Net(BayesianNet):          # the mixture is the prior of a latent that a Normal drew
            def forward(self, observed):
                self.observe(observed)
                self.normal_mixture("z", lg, mu, logstd=ls, batch_shape=(B,), n_samples=K)
                return self
        q = zs.distributions.Normal(x.detach().view(K, B, D), logstd=torch.full((K, B, D), -60.0, device=device, dtype=dtype))
        z = q.sample()          # std = e^-60: the draw is its mean to the last bit
        assert torch.equal(z, x.detach().view(K, B, D))
        x = z.requires_grad_(True)
        net = Net(device=torch.device(device))({"z": x})
        lp, dist = net.nodes["z"].log_prob(), net.nodes["z"].dist
        assert tuple(net.log_joint().shape) == (K, B)
    else:
        dist = NormalMixture(lg, mu, **({"logstd": ls} if scale == "logstd" else {"std": torch.exp(ls)}))
        lp = dist.log_prob(x.view(K, B, D))
    grads = torch.autograd.grad((lp.reshape(-1) * g.to(device, dtype)).sum(), [x, lg, mu, ls])
    t = truth(*ins)
    for name, got, tol in zip(NAMES, (lp,) + grads, bounds(dtype, *ins, t)):
        err = (got.detach().cpu().to(F64).reshape(t[name].shape) - t[name]).abs()
        print("%s: worst error / tolerance = %.3f" % (name, float((err / tol).max())))
        assert bool((err <= tol).all()), name
    return dist


@pytest.mark.parametrize("dtype,scale", [(F32, "logstd"), (F64, "logstd"), (F64, "std")])
def test_cpu_tensors_run_the_torch_composition(dtype, scale):
    dist = check_against_truth("cpu", dtype, scale=scale)
    assert dist.last_path["path"].startswith("torch composition") and "CPU" in zs.explain(dist)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64])
def test_prior_node_in_a_bayesian_net_runs_the_kernels(dtype):
    dist = check_against_truth("cuda:0", dtype, via_bn=True)
    assert dist.last_path["path"].startswith("zs_mix_prepare + zs_mix_logprob") and dist.last_path["why"] is None
    wide = check_against_truth("cuda:0", dtype, D=65)
    assert wide.last_path["path"].startswith("torch composition") and "wider than 64" in zs.explain(wide)


@pytest.mark.gpu
@pytest.mark.parametrize("wants", [(True, False), (False, True)])
def test_only_the_gradient_that_is_needed_is_launched(wants):
    lg, mu, ls, x, _ = (a.to("cuda:0", F32) for a in case_inputs(D, C, K * B))
    x.requires_grad_(wants[0])
    for p in (lg, mu, ls):
        p.requires_grad_(wants[1])
    dist = NormalMixture(lg, mu, logstd=ls)
    dist.log_prob(x).sum().backward()
    ws = dist.last_workspaces
    assert ws["needs_input_grad"] == (wants[1],) * 3 + (wants[0],)
    assert (ws["grad_x_ran"], ws["grad_params_workspace_elems"] is not None) == wants
    assert ws["grad_params_workspace_elems"] is None or ws["grad_params_workspace_elems"] > 0
    assert (x.grad is not None, lg.grad is not None, mu.grad is not None, ls.grad is not None) == (wants[0],) + (wants[1],) * 3


@pytest.mark.gpu
def test_samples_follow_the_weights_and_the_component():
    lg = torch.zeros(C, device="cuda:0")
    lg[3] += 80.0
    mu = case_inputs(D, C, 1)[1].to("cuda:0", F32)
    z = NormalMixture(lg, mu, std=torch.full_like(mu, 1e-3), batch_shape=(64,)).sample(8)
    assert tuple(z.shape) == (8, 64, D) and bool(((z - mu[3]).abs() < 1e-2).all())
