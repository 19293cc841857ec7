"""AdmixtureMultinomial and ``BayesianNet.admixture_multinomial`` (zhusuan/distributions/admixture.py): the public interface
over the kernels of include/zs_topic.h.  The truth and the bounds are those of tests/test_topic_kernel.py."""
import os
import subprocess
import sys

import pytest
import torch

import zhusuan as zs
from zhusuan.distributions import AdmixtureMultinomial
from zhusuan.framework.bn import BayesianNet
from test_topic_kernel import bounds, case_inputs, truth

F32, F64 = torch.float32, torch.float64


def test_import_loads_neither_the_binding_nor_the_library():
    code = ("import sys, zhusuan; assert 'zhusuan._topic_hip' not in sys.modules; "
            "from zhusuan.distributions import AdmixtureMultinomial; assert 'zhusuan._topic_hip' not in sys.modules; "
            "from zhusuan import _topic_hip; assert _topic_hip._LIB is None")
    pkg_root = os.path.dirname(os.path.dirname(os.path.abspath(zs.__file__)))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=pkg_root, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr


def test_construction_shapes_and_errors():
    d = AdmixtureMultinomial(torch.zeros(3, 5, 4), torch.zeros(4, 7), device="cpu")
    assert tuple(d.batch_shape) == (3, 5) and d.n_topics == 4 and d.n_words == 7 and d.dtype == F32
    for shape in ((5, 7), (3, 5, 7), (7,)):          # shared over the chains, full, shared over everything
        assert tuple(d.log_prob(torch.ones(shape)).shape) == (3, 5)
    assert tuple(AdmixtureMultinomial(torch.zeros(3, 5, 4), torch.zeros(4, 7), group_ndims=1, device="cpu").log_prob(torch.ones(5, 7)).shape) == (3,)
    with pytest.raises(ValueError, match=r"\[4, V\].*\(5, 7\)"):
        AdmixtureMultinomial(torch.zeros(3, 4), torch.zeros(5, 7), device="cpu")
    with pytest.raises(ValueError, match=r"\(3, 5\).*V = 7.*\(3, 7\)"):
        d.log_prob(torch.ones(3, 7))
    with pytest.raises(ValueError, match=r"\(5, 8\)"):
        d.log_prob(torch.ones(5, 8))
    with pytest.raises(NotImplementedError, match="cannot be sampled"):
        d.sample()

    class Net(BayesianNet):
        def forward(self, observed):
            self.observe(observed)
            self.admixture_multinomial("words", torch.zeros(5, 4), torch.zeros(4, 7))

    with pytest.raises(NotImplementedError, match="node 'words' cannot be sampled"):
        Net()({})


def check_against_truth(device, dtype, K=5, V=65, via_bn=False):
    """log_prob / log_joint and autograd.grad with respect to eta and beta at (3, 5, K, V) against the float64 truth, within
    the kernel test's bounds for `dtype`; returns the distribution."""
    H, B, X, _ = case_inputs(K, V, 3, 5, False)
    eta = H.view(3, 5, K).to(device, dtype).clone().requires_grad_(True)
    beta = B.to(device, dtype).clone().requires_grad_(True)
    x = X.to(device, dtype)
    if via_bn:
        class Net(BayesianNet):
            def forward(self, observed):
                self.observe(observed)
                self.admixture_multinomial("x", eta, beta)
                return self
        net = Net(device=torch.device(device))({"x": x})
        lp, dist = net.log_joint(), net.nodes["x"].dist
    else:
        dist = AdmixtureMultinomial(eta, beta)
        lp = dist.log_prob(x)
    g = torch.linspace(-1.0, 1.0, 15, dtype=F64)
    d_eta, d_beta = torch.autograd.grad((lp.reshape(-1) * g.to(device, dtype)).sum(), [eta, beta])
    t = truth(H, B, X, g)
    for name, got, tol in zip(("lp", "dH", "dB"), (lp, d_eta, d_beta), bounds(dtype, H, B, g, t)):
        err = (got.detach().cpu().to(F64).reshape(t[name].shape) - t[name]).abs()
        print("%s: worst error / tolerance = %.3f" % (name, float((err / tol).max())))
        assert bool((err <= tol).all()), name
    return dist


@pytest.mark.parametrize("dtype", [F32, F64])
def test_cpu_tensors_run_the_torch_composition(dtype):
    dist = check_against_truth("cpu", dtype)
    assert dist.last_path["path"].startswith("torch composition") and "CPU" in zs.explain(dist)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64])
def test_observed_node_in_a_bayesian_net_runs_the_kernels(dtype):
    dist = check_against_truth("cuda:0", dtype, via_bn=True)
    assert dist.last_path["path"].startswith("zs_topic_prepare + zs_topic_logprob") and dist.last_path["why"] is None
    wide = check_against_truth("cuda:0", dtype, K=129, V=17)
    assert wide.last_path["path"].startswith("torch composition") and "128 topics" in zs.explain(wide)


@pytest.mark.gpu
@pytest.mark.parametrize("wants", [(True, False), (False, True)])
def test_only_the_gradient_that_is_needed_is_launched(wants):
    H, B, X, _ = case_inputs(5, 65, 3, 5, False)
    eta = H.view(3, 5, 5).to("cuda:0", F32).requires_grad_(wants[0])
    beta = B.to("cuda:0", F32).requires_grad_(wants[1])
    dist = AdmixtureMultinomial(eta, beta)
    dist.log_prob(X.to("cuda:0", F32)).sum().backward()
    ws = dist.last_workspaces
    assert ws["needs_input_grad"] == wants
    assert (ws["grad_doc_workspace_elems"] is not None, ws["grad_topic_workspace_elems"] is not None) == wants
    assert all(n is None or n > 0 for n in (ws["grad_doc_workspace_elems"], ws["grad_topic_workspace_elems"]))
    assert (eta.grad is not None, beta.grad is not None) == wants
