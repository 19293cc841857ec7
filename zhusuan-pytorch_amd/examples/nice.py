"""NICE (additive couplings + a scaling layer under a Logistic base) on synthetic MNIST-shaped data.

Counterpart of the reference caller examples/normlizing_flows/nice_mnist.py:13-92: the same ``BayesianNet`` with one
``FlowDistribution`` node scored with ``n_samples=-1``, the same flow (``num_coupling`` ``MaskCoupling`` layers on alternating
odd/even masks, then ``Scaling``), the same loss ``-log_prob(x).mean()`` and optimiser settings.  Around every inner network
the split and the merge are one launch each, the scaling and the log-density tail one each (include/zs_flow.h).
Differences: the data are synthetic uniform "dequantised pixels" (the reference downloads MNIST), and the masks and the base
distribution's parameters are created on the model's device."""
import argparse
import time

import torch

from zhusuan.framework.bn import BayesianNet
from zhusuan.distributions import Logistic, FlowDistribution
from zhusuan.invertible import get_coupling_mask, MaskCoupling, Scaling, RevSequential


class NICE(BayesianNet):
    def __init__(self, num_coupling, in_out_dim, mid_dim, hidden, device='cuda'):
        super(NICE, self).__init__()
        device = torch.device(device)
        self.in_out_dim = in_out_dim
        couplings = [MaskCoupling(in_out_dim=in_out_dim, mid_dim=mid_dim, hidden=hidden, mask=m.to(device))
                     for m in get_coupling_mask(in_out_dim, 1, num_coupling)]
        self.flow = RevSequential(couplings + [Scaling(in_out_dim)])
        base = Logistic(loc=torch.zeros([in_out_dim], device=device), scale=torch.ones([in_out_dim], device=device))
        # n_samples=-1: the node is never sampled at creation, only scored (a property of FlowDistribution alone)
        self.sn(FlowDistribution(latents=base, transformation=self.flow, device=device), name="x", n_samples=-1)

    def sample(self, size):
        return self.nodes["x"].dist.sample(size)

    def forward(self, x):
        return self.nodes['x'].log_prob(x)


def build(num_coupling=4, in_out_dim=784, mid_dim=1000, hidden=5, device='cuda'):
    """The reference's sizes by default (nice_mnist.py:45-50)."""
    return NICE(num_coupling, in_out_dim, mid_dim, hidden, device=device).to(device)


def train(model, x_all, batch, steps, lr=1e-3, log=None):
    """``steps`` Adam steps (nice_mnist.py:58: eps=1e-4) over minibatches of ``x_all``; returns the losses as floats."""
    opt = torch.optim.Adam(model.parameters(), lr=lr, eps=1e-4)
    n_batches = max(x_all.shape[0] // batch, 1)
    losses = []
    for step in range(steps):
        i = (step % n_batches) * batch
        opt.zero_grad()
        loss = -model(x_all[i:i + batch]).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if log and (step + 1) % 50 == 0:
            log("step %d  loss %.4f" % (step + 1, losses[-1]))
    return losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=200)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--samples', type=int, default=64)
    args = ap.parse_args()
    device = torch.device('cuda')
    model = build(device=device)
    g = torch.Generator().manual_seed(1234)
    x_all = torch.rand(args.batch * 8, model.in_out_dim, generator=g).to(device)
    t0 = time.time()
    train(model, x_all, args.batch, args.steps, log=print)
    torch.cuda.synchronize()
    print("%.1f steps/s" % (args.steps / (time.time() - t0)))
    with torch.no_grad():
        samples = model.sample(args.samples)
    print("samples", tuple(samples.shape), "mean %.4f" % float(samples.mean()))


if __name__ == '__main__':
    main()
