"""A Bayesian linear-ReLU network whose WHOLE weight vector has one low-rank Gaussian posterior (synthetic regression data).

q(w) = MultivariateNormalLowRank(mean [D], cov_factor [D, r], cov_diag [D]) over the D = in * hidden + hidden weights, flat: the
draw, its density and their gradients run on the kernels of include/zs_lowrank.h (``zhusuan.explain(node.dist)`` names them); the package has no CPU path
for the other nodes, so the example needs a HIP device.  Trained by the reparameterised ELBO.

    python examples/bnn_lowrank.py [--steps 200] [--rank 8] [--hidden 50] [--particles 10]"""
import argparse

import torch

import zhusuan as zs
from zhusuan.framework.bn import BayesianNet
from zhusuan.variational.elbo import ELBO


class Net(BayesianNet):
    def __init__(self, build):
        super().__init__()
        self.build = build

    def forward(self, observed):
        self.observe(observed)
        self.build(self)
        return self


def build(n_in=8, hidden=50, rank=8, particles=10, n_data=256, device=torch.device("cuda:0"), seed=0):
    """(objective, parameters, observed): the ELBO of the network over synthetic data."""
    g = torch.Generator().manual_seed(seed)
    D = n_in * hidden + hidden
    x = torch.randn(n_data, n_in, generator=g).to(device)
    y = torch.sin(x.sum(-1)).to(device)
    params = dict(mean=0.1 * torch.randn(D, generator=g), factor=0.01 * torch.randn(D, rank, generator=g), logd=torch.full((D,), -3.0))
    params = {k: v.to(device).requires_grad_(True) for k, v in params.items()}

    def q(net):
        net.multivariate_normal_low_rank('w', params['mean'], params['factor'], torch.exp(params['logd']), n_samples=particles)

    def p(net):
        w = net.normal('w', mean=torch.zeros(D, device=device), std=torch.ones(D, device=device), n_samples=particles, group_ndims=1)
        w1, w2 = w[:, :n_in * hidden].reshape(-1, n_in, hidden), w[:, n_in * hidden:]
        h = torch.relu(torch.einsum("ni,kih->knh", x, w1))
        net.normal('y', mean=torch.einsum("knh,kh->kn", h, w2), std=0.1 * torch.ones(n_data, device=device), group_ndims=1)
    return ELBO(Net(p).to(device), Net(q).to(device), estimator="sgvb").to(device), params, {'y': y}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rank", type=int, default=8)
    ap.add_argument("--hidden", type=int, default=50)
    ap.add_argument("--particles", type=int, default=10)
    a = ap.parse_args()
    device = torch.device("cuda:0")
    objective, params, observed = build(hidden=a.hidden, rank=a.rank, particles=a.particles, device=device)
    opt = torch.optim.Adam(list(params.values()), lr=1e-2)
    for step in range(a.steps):
        opt.zero_grad()
        loss = objective(observed)
        loss.backward()
        opt.step()
        if step % 50 == 0 or step == a.steps - 1:
            print("step %4d  -ELBO %.3f" % (step, float(loss.detach())))
    print("posterior: %s" % zs.explain(objective.variational.nodes['w'].dist))


if __name__ == "__main__":
    main()
