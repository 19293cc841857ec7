"""Shared by the sampler tests and by tests/golden/mcmc/gen_mcmc_golden.py (a helper, not a test): the small BNN of the
fixtures, written once against the BayesianNet interface, so that the generator builds it on the reference's class and the
tests on this package's.  Shape of the reference caller examples/bayesian_neural_nets/bnn_sgmcmc.py:16-70: a Normal prior
node per weight matrix (``group_ndims=2``, K particles, ``reduce_mean_dims=[0]``), the particle-batched network in plain
torch ops, a Normal likelihood with ``reduce_mean_dims=[0, 1]`` and a multiplier."""
import math

import numpy as np
import torch

N_PARTICLES, N_ROWS, Y_LOGSTD, MULTIPLIER, LR, N_UPDATES = 3, 6, -1.0, 24, 1e-3, 6
# name -> (sampler class name, constructor keywords, layer sizes)
CASES = {
    "sgld": ("SGLD", {}, [3, 4, 1]),
    "psgld": ("PSGLD", {}, [3, 4, 1]),
    "sghmc_first_order": ("SGHMC", dict(friction=0.3, variance_estimate=0.02, n_iter_resample_v=3, second_order=False), [3, 1]),
    "sghmc_second_order": ("SGHMC", dict(friction=0.3, variance_estimate=0.02, n_iter_resample_v=3, second_order=True), [3, 1]),
}


def make_net(BayesianNet, layer_sizes, dtype=torch.float32, device=torch.device("cpu"), n_particles=N_PARTICLES,
             y_logstd=Y_LOGSTD, multiplier=MULTIPLIER):
    class Net(BayesianNet):
        def __init__(self):
            super().__init__()
            self.y_logstd = torch.full([1], y_logstd, dtype=dtype, device=device)
            self.w_means = [torch.zeros([n_out, n_in + 1], dtype=dtype, device=device)
                            for n_in, n_out in zip(layer_sizes[:-1], layer_sizes[1:])]
            self.w_logstds = [torch.zeros([n_out, n_in + 1], dtype=dtype, device=device)
                              for n_in, n_out in zip(layer_sizes[:-1], layer_sizes[1:])]

        def forward(self, observed):
            self.observe(observed)
            x = self.observed['x']
            h = x.unsqueeze(0).expand(n_particles, *x.shape)
            for i in range(len(layer_sizes) - 1):
                w = self.normal(name='w' + str(i), mean=self.w_means[i], logstd=self.w_logstds[i], group_ndims=2,
                                n_samples=n_particles, reduce_mean_dims=[0])
                h = torch.cat([h, torch.ones([*h.shape[:-1], 1], dtype=dtype, device=device)], -1)
                p = math.sqrt(h.shape[2])
                h = torch.matmul(w.unsqueeze(1), h.unsqueeze(-1)).squeeze(-1) / p
                if i < len(layer_sizes) - 2:
                    h = torch.relu(h)
            y_mean = torch.squeeze(h, 2)
            y = self.observed['y']
            self.cache['rmse'] = torch.sqrt(torch.mean((y - torch.mean(y_mean, 0)) ** 2))
            self.normal(name='y', mean=y_mean, logstd=self.y_logstd, reduce_mean_dims=[0, 1], multiplier=multiplier)
            return self

    return Net().to(device)          # (a net without parameters takes its nodes' device from here)


def make_data(seed, n_in):
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((N_ROWS, n_in)).astype(np.float32)
    y = (x.sum(1) * 0.5 + 0.1 * rng.standard_normal(N_ROWS)).astype(np.float32)
    return x, y
