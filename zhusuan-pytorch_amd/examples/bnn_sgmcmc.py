"""Bayesian neural network regression with stochastic-gradient MCMC on synthetic UCI-sized data.

Counterpart of the reference caller examples/bayesian_neural_nets/bnn_sgmcmc.py:16-135: the weights of every layer are latent
Normal nodes (``group_ndims=2``, K particles = K parallel chains, ``reduce_mean_dims=[0]``), the likelihood is a Normal with a
fixed ``y_logstd = -1.95`` and ``multiplier`` = training-set size, and a sampler of ``zhusuan.mcmc`` moves all weights once per
minibatch: one ``autograd.grad`` of the log joint through the particle-batched network (``examples.bnn_vi.Net``: PM1 / PL1 of
include/zs_hip.h) and ONE fused update launch over both weight tensors (include/zs_mcmc.h).  The test error is the RMSE of the
prediction averaged over the K current samples, as in the reference's evaluation (:136-142).  The reference's loop also
re-estimates the prior's log-std from the samples after every step (:124-127); the prior is kept fixed here."""
import argparse
import time

import torch

from zhusuan.mcmc import SGLD, PSGLD, SGHMC

from examples import bnn_vi


class Net(bnn_vi.Net):
    def __init__(self, layer_sizes, n_particles, multiplier=456, layer=None):
        super().__init__(layer_sizes, n_particles, multiplier, layer=layer)
        del self.y_logstd                                    # fixed here, learned in bnn_vi (bnn_sgmcmc.py:21-22)
        self.register_buffer('y_logstd', torch.full([1], -1.95))


def make_sampler(name, lr):
    if name == 'sgld':
        return SGLD(lr)
    if name == 'psgld':
        return PSGLD(lr)
    if name == 'sghmc':
        return SGHMC(lr, friction=0.3, variance_estimate=0.02, n_iter_resample_v=50, second_order=True)
    raise ValueError("sampler: 'sgld', 'psgld' or 'sghmc'")


def run(steps=200, batch=114, particles=20, layer_sizes=(13, 50, 1), sampler='sgld', lr=1e-3, device='cuda', layer=None,
        n_train=456, n_test=50, seed=1234, log=None):
    """`steps` sampler calls (the first one draws the chains' starting points from the prior) on minibatches of a synthetic
    regression problem; returns the test RMSE of the prediction averaged over the K current samples (a float)."""
    device = torch.device(device)
    g = torch.Generator().manual_seed(seed)
    n_in = layer_sizes[0]
    w_true = torch.randn(n_in, generator=g) / n_in ** 0.5
    x_all = torch.randn(n_train + n_test, n_in, generator=g)
    y_all = torch.tanh(x_all @ w_true) + 0.1 * torch.randn(n_train + n_test, generator=g)
    x_train, y_train = x_all[:n_train].to(device), y_all[:n_train].to(device)
    x_test, y_test = x_all[n_train:].to(device), y_all[n_train:].to(device)
    net = Net(list(layer_sizes), particles, multiplier=n_train, layer=layer).to(device)
    model = make_sampler(sampler, lr).to(device)
    batch = min(batch, n_train)
    n_batches = max(n_train // batch, 1)
    rmse = float('nan')
    for step in range(steps):
        b = step % n_batches
        obs = {'x': x_train[b * batch:(b + 1) * batch], 'y': y_train[b * batch:(b + 1) * batch]}
        w_samples = model.sample(net, obs, resample=(step == 0))
        if (step + 1) % 50 == 0 or step == steps - 1:
            net.forward({**dict((k, w.detach()) for k, w in w_samples.items()), 'x': x_test, 'y': y_test})
            rmse = float(net.cache['rmse'])
            if log:
                log("step %d  test rmse %.4f" % (step + 1, rmse))
    return rmse


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=114)
    ap.add_argument('--particles', type=int, default=20)
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--sampler', default='sgld', choices=['sgld', 'psgld', 'sghmc'])
    ap.add_argument('--lr', type=float, default=1e-3)
    args = ap.parse_args()
    t0 = time.time()
    rmse = run(steps=args.steps, batch=args.batch, particles=args.particles, sampler=args.sampler, lr=args.lr, log=print)
    torch.cuda.synchronize()
    print("test rmse %.4f  %.1f sampler steps/s" % (rmse, args.steps / (time.time() - t0)))


if __name__ == '__main__':
    main()
