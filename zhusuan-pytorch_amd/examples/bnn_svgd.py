"""Bayesian neural network regression with Stein variational gradient descent on synthetic UCI-sized data.

The model of examples/bnn_sgmcmc.py with the sampler swapped: the weights of every layer are latent Normal nodes
(``group_ndims=2``, K particles), the likelihood a Normal with a fixed ``y_logstd = -1.95`` and ``multiplier`` = training-set size,
the network itself one launch (``zhusuan.particle_mlp``).  The one difference is what SVGD needs: the log joint keeps the particle
axis (the likelihood is averaged over the minibatch only, the prior not over the particles), so ``bn.log_joint()`` is [K] and its
gradient is each particle's own.  ``zhusuan.mcmc.SVGD`` then moves all K particles of both weight tensors at once: one
``autograd.grad`` and three launches of lib/libzs_svgd.so a step (include/zs_svgd.h).  The test error is the RMSE of the
prediction averaged over the K particles."""
import argparse
import time

import torch

import zhusuan
from zhusuan.framework.bn import BayesianNet
from zhusuan.mcmc import SVGD


class Net(BayesianNet):
    def __init__(self, layer_sizes, n_particles, multiplier=456):
        super().__init__()
        self.layer_sizes = list(layer_sizes)
        self.n_particles = n_particles
        self.multiplier = multiplier
        self.register_buffer('y_logstd', torch.full([1], -1.95))

    def forward(self, observed):
        self.observe(observed)
        x, y, dev = self.observed['x'], self.observed['y'], self.observed['x'].device
        ws = [self.normal(name='w' + str(i), mean=torch.zeros([n_out, n_in + 1], device=dev), std=torch.ones([n_out, n_in + 1], device=dev),
                          group_ndims=2, n_samples=self.n_particles)
              for i, (n_in, n_out) in enumerate(zip(self.layer_sizes[:-1], self.layer_sizes[1:]))]
        y_mean = torch.squeeze(zhusuan.particle_mlp(x, ws), 2)
        self.cache['rmse'] = zhusuan.particle_rmse(y_mean, y)
        self.normal(name='y', mean=y_mean, logstd=self.y_logstd, reduce_mean_dims=[1], multiplier=self.multiplier)
        return self


def run(steps=200, batch=114, particles=20, layer_sizes=(13, 50, 1), step_size=1e-3, adagrad=True, device='cuda', n_train=456,
        n_test=50, seed=1234, log=None):
    """`steps` SVGD steps from particles drawn from the prior, on minibatches of a synthetic regression problem; returns
    (the test RMSE of the prediction averaged over the K particles, the sampler)."""
    device = torch.device(device)
    g = torch.Generator().manual_seed(seed)
    n_in = layer_sizes[0]
    w_true = torch.randn(n_in, generator=g) / n_in ** 0.5
    x_all = torch.randn(n_train + n_test, n_in, generator=g)
    y_all = torch.tanh(x_all @ w_true) + 0.1 * torch.randn(n_train + n_test, generator=g)
    x_train, y_train = x_all[:n_train].to(device), y_all[:n_train].to(device)
    x_test, y_test = x_all[n_train:].to(device), y_all[n_train:].to(device)
    net = Net(layer_sizes, particles, multiplier=n_train).to(device)
    svgd = SVGD(step_size=step_size, adagrad=adagrad)
    batch = min(batch, n_train)
    n_batches = max(n_train // batch, 1)
    net.forward({'x': x_train[:batch], 'y': y_train[:batch]})
    latent = {k: v.tensor.detach() for k, v in net.nodes.items() if k not in ('x', 'y')}
    rmse = float('nan')
    for step in range(steps):
        b = step % n_batches
        obs = {'x': x_train[b * batch:(b + 1) * batch], 'y': y_train[b * batch:(b + 1) * batch]}
        latent, info = svgd.sample(net, obs, latent, inplace=True)
        if (step + 1) % 50 == 0 or step == steps - 1:
            net.forward({**latent, 'x': x_test, 'y': y_test})
            rmse = float(net.cache['rmse'])
            if log:
                log("step %d  test rmse %.4f  bandwidth %.3f  (%s)" % (step + 1, rmse, float(info.bandwidth), svgd.last_path["path"]))
    return rmse, svgd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=114)
    ap.add_argument('--particles', type=int, default=20)
    ap.add_argument('--steps', type=int, default=2000)
    ap.add_argument('--step-size', type=float, default=1e-3)
    ap.add_argument('--plain', action='store_true', help="no AdaGrad preconditioner")
    args = ap.parse_args()
    t0 = time.time()
    rmse, _ = run(steps=args.steps, batch=args.batch, particles=args.particles, step_size=args.step_size, adagrad=not args.plain, log=print)
    torch.cuda.synchronize()
    print("test rmse %.4f  %.1f SVGD steps/s" % (rmse, args.steps / (time.time() - t0)))


if __name__ == '__main__':
    main()
