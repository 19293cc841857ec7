"""``zhusuan.distributions.FlowDistribution`` on both back-ends: log_prob, sample, ``n_samples=-1`` inside a BayesianNet, the
one-launch tail against the unfused path on the same inputs, a base that takes the unfused path, and the errors.

Tolerance (float32): the tail sums D <= 7 log-densities of order 1-10 and a log-det; fused and unfused evaluate the same
formula with differently rounded elementary functions (<= 4 ulp each) and another summation order: (D + 8) 2^-24 of the
summed magnitudes (< 100) stays below 1e-4; gradients likewise."""
import pytest
import torch

import flow_host
from flow_host import fdev  # noqa: F401
from test_flow_layers import close


def _nice(D, dev, base="logistic", seed=0):
    from zhusuan.distributions import Logistic, Normal, Laplace, FlowDistribution
    from zhusuan.invertible import get_coupling_mask, MaskCoupling, Scaling, RevSequential
    torch.manual_seed(seed)
    masks = get_coupling_mask(D, 1, 3)
    flow = RevSequential([MaskCoupling(D, 5, 2, masks[i].to(dev)) for i in range(3)] + [Scaling(D)]).to(dev)
    with torch.no_grad():
        flow.layers[-1].log_scale.normal_()
    loc, scale = torch.linspace(-0.5, 0.5, D, device=dev), torch.linspace(0.5, 1.5, D, device=dev)
    if base == "logistic":
        dis = Logistic(loc=loc, scale=scale)
    elif base == "normal":
        dis = Normal(mean=loc, std=scale)
    else:
        dis = Laplace(loc=loc, scale=scale)
    return flow, dis, FlowDistribution(latents=dis, transformation=flow)


def _unfused(flow, dis, x):
    z, ld = flow(x, reverse=False)
    return torch.sum(dis.log_prob(z), dim=1) + ld


@pytest.mark.parametrize("base", ["logistic", "normal"])
@pytest.mark.parametrize("B,D", [(1, 2), (5, 7)])
def test_fused_tail_equals_the_unfused_path(fdev, base, B, D):
    import zhusuan as zs
    flow, dis, fd = _nice(D, fdev, base)
    assert fd.is_reparameterized is False and fd.is_continuous
    x = torch.rand(B, D, generator=torch.Generator().manual_seed(B), dtype=torch.float32).to(fdev)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    with flow_host.count_launches() as c:
        lp = fd.log_prob(xa)
    assert c["tail"] == 1 and lp.shape == (B,)
    assert "zs_flow_tail" in zs.explain(fd)
    ref = _unfused(flow, dis, xb)
    close(lp, ref, torch.float32, "log_prob")
    w = torch.linspace(0.5, 1.5, B, device=fdev)
    for p in flow.parameters():
        p.grad = None
    with flow_host.count_launches() as c:
        (lp * w).sum().backward()
    assert c["tail_bwd"] == 1
    got = [xa.grad.clone()] + [p.grad.clone() for p in flow.parameters()]
    for p in flow.parameters():
        p.grad = None
    (ref * w).sum().backward()
    want = [xb.grad] + [p.grad for p in flow.parameters()]
    for a, b in zip(got, want):
        close(a, b, torch.float32, "gradient")


def test_tail_with_row_parameters_and_row_log_det(fdev):
    """[B, D] parameters and a [B] log-det (a transformation that reports one per row)."""
    from zhusuan.distributions import Normal, FlowDistribution
    from zhusuan.invertible import RevNet

    class RowScale(RevNet):
        def __init__(self):
            super().__init__()
            self.a = torch.nn.Parameter(torch.tensor(0.3))

        def _forward(self, x, **kw):
            s = self.a * x.sum(1, keepdim=True)
            return x * torch.exp(s), (s * x.shape[1]).squeeze(1)
    B, D = 4, 3
    t = RowScale().to(fdev)
    mean, std = torch.rand(B, D, device=fdev), torch.rand(B, D, device=fdev) + 0.5
    fd = FlowDistribution(Normal(mean=mean, std=std), t)
    x = torch.rand(B, D, device=fdev)
    with flow_host.count_launches() as c:
        lp = fd.log_prob(x)
    assert c["tail"] == 1
    z, ld = t(x)
    ref = torch.sum(Normal(mean=mean, std=std).log_prob(z), dim=1) + ld
    close(lp, ref, torch.float32)
    with flow_host.count_launches() as c:
        g1, = torch.autograd.grad(lp.sum(), t.a)
    assert c["tail_bwd"] == 1
    g2, = torch.autograd.grad(ref.sum(), t.a)
    close(g1, g2, torch.float32)


def test_a_base_without_a_fused_tail_takes_the_reference_ops(fdev):
    import zhusuan as zs
    flow, dis, fd = _nice(6, fdev, "laplace")
    x = torch.rand(3, 6, device=fdev)
    with flow_host.count_launches() as c:
        lp = fd.log_prob(x.clone())
    assert c["tail"] == 0 and "Laplace" in zs.explain(fd) and "reference ops" in zs.explain(fd)
    close(lp, _unfused(flow, dis, x.clone()), torch.float32)
    # parameters of the base that require grad: unfused as well, and they receive their gradient
    from zhusuan.distributions import Normal, FlowDistribution
    mean = torch.zeros(6, device=fdev, requires_grad=True)
    fd2 = FlowDistribution(Normal(mean=mean, std=torch.ones(6, device=fdev)), flow)
    with flow_host.count_launches() as c:
        fd2.log_prob(x.clone()).sum().backward()
    assert c["tail"] == 0 and mean.grad is not None and "requires grad" in zs.explain(fd2)


def test_sample_and_the_unsampled_node(fdev):
    from zhusuan.framework.bn import BayesianNet
    D = 6
    flow, dis, fd = _nice(D, fdev)
    assert fd.sample(-1) is None and fd._sample(-1) is None
    with torch.no_grad():
        s = fd.sample(3)
        assert s.shape == (3, D) and s.device.type == fdev.type and bool(torch.isfinite(s).all())
        # the sample is the inverse image of a base draw: pushing it forward and scoring it is finite and of shape [3]
        assert fd.log_prob(s.clone()).shape == (3,)

    class Net(BayesianNet):
        def __init__(self):
            super().__init__()
            self.flow = flow
            self.sn(fd, name="x", n_samples=-1)

        def forward(self, x):
            return self.nodes["x"].log_prob(x)
    net = Net()
    x = torch.rand(4, D, device=fdev)
    lp = net(x.clone())
    close(lp, _unfused(flow, dis, x.clone()), torch.float32)
    (-lp.mean()).backward()
    assert flow.layers[-1].log_scale.grad.shape == (1, D)
    with torch.no_grad():
        assert net.nodes["x"].dist.sample(2).shape == (2, D)


def test_errors(fdev):
    from zhusuan.distributions import Normal, FlowDistribution
    from zhusuan.invertible import MADE
    with pytest.raises(NotImplementedError, match="outside the variational-inference hot path"):
        FlowDistribution(1.0, 1.0)
    with pytest.raises(NotImplementedError, match="zhusuan.invertible.RevNet"):
        FlowDistribution(Normal(mean=torch.zeros(3, device=fdev), std=torch.ones(3, device=fdev)), torch.nn.Linear(3, 3))
    # a bare MADE reports a [B, D] log-det: the add fails to broadcast, as in the reference
    made = MADE(6, 8, 1).to(fdev)
    fd = FlowDistribution(Normal(mean=torch.zeros(6, device=fdev), std=torch.ones(6, device=fdev)), made)
    with pytest.raises(RuntimeError):
        fd.log_prob(torch.rand(3, 6, device=fdev))
