"""Did the chains converge?  The diagonal Gaussian of examples/gaussian_hmc.py, sampled by several HMC chains whose draws after
warm-up go into a ``zhusuan.diagnostics.Trace`` on the device; the summary printed at the end -- mean, var+, split R-hat and
effective sample size of every coordinate -- is one kernel launch (include/zs_diag.h)."""
import argparse

import torch

from zhusuan.diagnostics import Trace
from zhusuan.mcmc import HMC

from .gaussian_hmc import Gaussian


def run(n_x=2, n_chains=4, n_iters=400, n_leapfrogs=10, step_size=0.1, device='cuda', seed=1, log=None):
    """``n_iters`` HMC iterations of ``n_chains`` chains from x = 0, the first half as warm-up with step-size adaptation.  Returns a
    dict: ``trace`` (the ``Trace`` of the draws after warm-up), ``summary`` (its ``Summary`` of 'x', every field ``[n_x]``, on the
    device), ``expected_std`` ``[n_x]`` (host) and ``step_size``."""
    device = torch.device(device)
    if device.type == 'cuda':
        torch.cuda.manual_seed(seed)
    warmup = n_iters // 2
    model = Gaussian(n_x, n_chains, device)
    sampler = HMC(step_size=step_size, n_leapfrogs=n_leapfrogs, adapt_step_size=True)
    latent = {'x': torch.zeros(n_chains, n_x, device=device)}
    trace = Trace(n_iters - warmup)
    for i in range(n_iters):
        if i == warmup:
            sampler.adapt_step_size = False
        latent, info = sampler.sample(model, {}, latent)
        if i >= warmup:
            trace.append(latent)
        if log and (i + 1) % 100 == 0:
            log("iteration %d  step size %.4f  acceptance %.3f" % (i + 1, sampler.step_size, float(info.acceptance_rate.mean())))
    summary = trace.summary(chain_ndims=1)['x']
    return dict(trace=trace, summary=summary, expected_std=1.0 / (torch.arange(n_x, dtype=torch.float64) + 1.0), step_size=sampler.step_size)


def report(r, log=print):
    s = r['summary']
    log("%4s %10s %10s %10s %8s %10s %5s" % ("x", "mean", "std", "expected", "rhat", "ess", "lags"))
    for j in range(s.mean.numel()):
        log("%4d %10.4f %10.4f %10.4f %8.4f %10.1f %5d%s" % (j, float(s.mean[j]), float(s.var[j]) ** 0.5, float(r['expected_std'][j]),
                                                              float(s.rhat[j]), float(s.ess[j]), int(s.lags[j]), " (capped)" if int(s.capped[j]) else ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n_x', type=int, default=2)
    ap.add_argument('--chains', type=int, default=4)
    ap.add_argument('--iters', type=int, default=400)
    ap.add_argument('--leapfrogs', type=int, default=10)
    ap.add_argument('--step_size', type=float, default=0.1)
    args = ap.parse_args()
    r = run(n_x=args.n_x, n_chains=args.chains, n_iters=args.iters, n_leapfrogs=args.leapfrogs, step_size=args.step_size, log=print)
    print("%d draws of %d chains after warm-up, step size %.4f" % (len(r['trace']), args.chains, r['step_size']))
    report(r)


if __name__ == '__main__':
    main()
