"""Bayesian neural network regression with a matrix-variate Gaussian posterior (Louizos & Welling 2016; Sun et al. 2017) on
synthetic UCI-sized data: examples/bnn_vi.py with, per layer, ``MatrixVariateNormalCholesky(mean, u_tril, v_tril)`` over the
``[n_in + 1, n_out]`` weight matrix in place of the fully factorised normal -- correlated weights for ``(n_in + 1)^2 + n_out^2``
covariance parameters.  The draw with its density is one launch of the matrix-core kernel M1 (include/zs_matvar.h), the backward a
main and a finish launch.  A layer with more inputs than the kernels take stays mean-field.
"""
import argparse
import math

import torch

from zhusuan.distributions import _matvar_functions
from zhusuan.framework.bn import BayesianNet
from zhusuan.variational.elbo import ELBO


class Net(BayesianNet):
    """Standard-normal priors over the weights, a Normal likelihood; the network is K batched GEMMs per layer."""

    def __init__(self, layer_sizes, n_particles, multiplier=456):
        super().__init__()
        self.layer_sizes, self.n_particles, self.multiplier = layer_sizes, n_particles, multiplier
        self.y_logstd = torch.nn.Parameter(torch.zeros([1], dtype=torch.float32))

    def forward(self, observed):
        self.observe(observed)
        x, K, dev = self.observed['x'], self.n_particles, self.device
        h = x.unsqueeze(0).expand(K, *x.shape)
        n_layers = len(self.layer_sizes) - 1
        for i, (n_in, n_out) in enumerate(zip(self.layer_sizes[:-1], self.layer_sizes[1:])):
            w = self.normal(name='w' + str(i), mean=torch.zeros([n_in + 1, n_out], device=dev), std=torch.ones([n_in + 1, n_out], device=dev),
                            group_ndims=2, n_samples=K, reduce_mean_dims=[0])
            h = torch.cat((h, torch.ones([*h.shape[:-1], 1], device=dev)), -1)
            h = torch.bmm(h, w) / math.sqrt(n_in + 1)
            if i < n_layers - 1:
                h = torch.relu(h)
        y_mean = torch.squeeze(h, 2)
        self.cache['rmse'] = torch.linalg.vector_norm(self.observed['y'] - y_mean.mean(0)) / math.sqrt(max(x.shape[0], 1))
        self.normal(name='y', mean=y_mean, logstd=self.y_logstd, reduce_mean_dims=[0, 1], multiplier=self.multiplier)
        return self


def factor(raw):
    """An unconstrained square matrix as a Cholesky factor: its strict lower triangle, the exponential of its diagonal."""
    return torch.tril(raw, -1) + torch.diag_embed(torch.exp(torch.diagonal(raw, dim1=-2, dim2=-1)))


class Variational(BayesianNet):
    def __init__(self, layer_sizes, n_particles):
        super().__init__()
        self.layer_sizes, self.n_particles = layer_sizes, n_particles
        cap = _matvar_functions.MAX_DIM[4]
        self.structured = [n_in + 1 <= cap and n_out <= cap for n_in, n_out in zip(layer_sizes[:-1], layer_sizes[1:])]
        shapes = [(n_in + 1, n_out) for n_in, n_out in zip(layer_sizes[:-1], layer_sizes[1:])]
        zeros = lambda *s: torch.nn.Parameter(torch.zeros(s, dtype=torch.float32))          # noqa: E731
        self.w_means = torch.nn.ParameterList([zeros(n, p) for n, p in shapes])
        # structured layers: the raw factors of the rows and of the columns (factor() below); the others: the log-stds, and a stub
        self.w_rows = torch.nn.ParameterList([zeros(n, n) if s else zeros(n, p) for (n, p), s in zip(shapes, self.structured)])
        self.w_cols = torch.nn.ParameterList([zeros(p, p) if s else zeros(1) for (n, p), s in zip(shapes, self.structured)])

    def forward(self, observed):
        self.observe(observed)
        for i, structured in enumerate(self.structured):
            if structured:
                self.matrix_variate_normal_cholesky('w' + str(i), self.w_means[i], factor(self.w_rows[i]), factor(self.w_cols[i]),
                                                    n_samples=self.n_particles, reduce_mean_dims=[0])
            else:
                self.normal(name='w' + str(i), mean=self.w_means[i], logstd=self.w_rows[i], group_ndims=2,
                            n_samples=self.n_particles, reduce_mean_dims=[0])
        return self


def build(layer_sizes=(13, 50, 1), n_particles=10, multiplier=456, device='cuda'):
    return ELBO(Net(list(layer_sizes), n_particles, multiplier), Variational(list(layer_sizes), n_particles)).to(device)


def run(layer_sizes=(13, 50, 1), n_particles=10, batch=114, steps=200, lr=1e-2, device='cuda', log_every=0):
    """Trains on synthetic data; returns the losses and the model."""
    device = torch.device(device)
    model = build(layer_sizes, n_particles, multiplier=batch, device=device)
    opt = torch.optim.Adam(model.parameters(), lr)
    g = torch.Generator().manual_seed(1234)
    x = torch.randn(batch, layer_sizes[0], generator=g).to(device)
    y = torch.sin(x[:, 0]) + 0.1 * torch.randn(batch, generator=g).to(device)
    losses = []
    for step in range(steps):
        loss = model({'x': x, 'y': y})
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss))
        if log_every and (step + 1) % log_every == 0:
            print("step %d  -ELBO %.4f  rmse %.4f" % (step + 1, losses[-1], float(model.generator.cache['rmse'])))
    return dict(losses=losses, model=model)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=114)
    ap.add_argument('--particles', type=int, default=10)
    ap.add_argument('--steps', type=int, default=200)
    args = ap.parse_args()
    run(n_particles=args.particles, batch=args.batch, steps=args.steps, log_every=50)


if __name__ == '__main__':
    main()
