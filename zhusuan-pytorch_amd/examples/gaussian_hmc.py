"""Sampling a diagonal Gaussian with Hamiltonian Monte Carlo.

Counterpart of the reference's examples/toy_examples/gaussian.py, run the way its "HMC parameters" block (``n_chains``,
``n_iters``, ``burnin``, ``n_leapfrogs = 20``) intended: the reference runs SGLD there because it ships no HMC.  The model is
the same -- ``x ~ Normal(0, stdev)`` with ``stdev = 1 / (1 .. n_x)`` -- written as a BayesianNet whose node holds one row per
chain (``group_ndims=1``: the log joint has one entry per chain).  The step size adapts during burn-in and is frozen after
it; the samples after burn-in give the mean and standard deviation printed at the end, as in the reference."""
import argparse
import time

import torch

from zhusuan.framework.bn import BayesianNet
from zhusuan.mcmc import HMC


class Gaussian(BayesianNet):
    def __init__(self, n_x, n_chains, device):
        super().__init__()
        stdev = 1.0 / (torch.arange(n_x, dtype=torch.float32) + 1.0)
        self.register_buffer('mean', torch.zeros(n_chains, n_x))
        self.register_buffer('std', stdev.expand(n_chains, n_x).contiguous())
        self.to(device)

    def forward(self, observed):
        self.observe(observed)
        self.normal('x', mean=self.mean, std=self.std, group_ndims=1)
        return self


def run(n_x=1, n_chains=1, n_iters=200, n_leapfrogs=20, step_size=0.1, device='cuda', seed=1, log=None):
    """``n_iters`` HMC iterations of ``n_chains`` chains from x = 0, the first half as burn-in with step-size adaptation.
    Returns a dict: ``samples`` [n_iters - burnin, n_chains, n_x] (on the device), ``mean``, ``std`` and ``expected_std`` [n_x]
    (host), ``acceptance`` (mean acceptance rate after burn-in) and ``step_size``."""
    device = torch.device(device)
    if device.type == 'cuda':
        torch.cuda.manual_seed(seed)
    burnin = n_iters // 2
    model = Gaussian(n_x, n_chains, device)
    sampler = HMC(step_size=step_size, n_leapfrogs=n_leapfrogs, adapt_step_size=True)
    latent = {'x': torch.zeros(n_chains, n_x, device=device)}
    samples, rate = [], torch.zeros((), device=device)
    for i in range(n_iters):
        if i == burnin:
            sampler.adapt_step_size = False
        latent, info = sampler.sample(model, {}, latent)
        if i >= burnin:
            samples.append(latent['x'])
            rate = rate + info.acceptance_rate.mean()
        if log and (i + 1) % 50 == 0:
            log("iteration %d  step size %.4f  acceptance %.3f" % (i + 1, sampler.step_size, float(info.acceptance_rate.mean())))
    samples = torch.stack(samples)
    flat = samples.reshape(-1, n_x).double()
    return dict(samples=samples, mean=flat.mean(0).cpu(), std=flat.std(0, unbiased=False).cpu(),
                expected_std=(1.0 / (torch.arange(n_x, dtype=torch.float64) + 1.0)), acceptance=float(rate) / max(n_iters - burnin, 1),
                step_size=sampler.step_size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n_x', type=int, default=1)
    ap.add_argument('--chains', type=int, default=1)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--leapfrogs', type=int, default=20)
    ap.add_argument('--step_size', type=float, default=0.1)
    args = ap.parse_args()
    t0 = time.time()
    r = run(n_x=args.n_x, n_chains=args.chains, n_iters=args.iters, n_leapfrogs=args.leapfrogs, step_size=args.step_size, log=print)
    print('Expected mean = {}'.format(torch.zeros(args.n_x).numpy()))
    print('Sample mean = {}'.format(r['mean'].numpy()))
    print('Expected stdev = {}'.format(r['expected_std'].numpy()))
    print('Sample stdev = {}'.format(r['std'].numpy()))
    print('Relative error of stdev = {}'.format(((r['std'] - r['expected_std']) / r['expected_std']).numpy()))
    print('acceptance %.3f  step size %.4f  %.1f iterations/s' % (r['acceptance'], r['step_size'], args.iters / (time.time() - t0)))


if __name__ == '__main__':
    main()
