"""A VAE / IWAE with a VampPrior (Tomczak & Welling 2018) on synthetic binarised data: the prior of the latent is the mixture of
the variational posteriors at C learned pseudo-inputs,

    p(z) = 1/C sum_c q(z | u_c),        mean_c, logstd_c = encoder(u_c),

a ``normal_mixture`` node with uniform logits whose parameters are re-computed from the encoder at every step.  Its density at
the posterior's draw, and the gradients that reach the draw, the pseudo-inputs and the encoder, come from the fused matrix-core
kernels of include/zs_mix.h: nothing of size ``[k batch, C]`` is kept for the backward.  Trained through the objectives as they
stand:

    k == 1   ELBO(estimator='sgvb')
    k  > 1   ImportanceWeightedObjective(axis=0, estimator='sgvb') with k particles
"""
import argparse

import torch
import torch.nn as nn

from zhusuan.framework.bn import BayesianNet
from zhusuan.variational.elbo import ELBO
from zhusuan.variational.importance_weighted_objective import ImportanceWeightedObjective
from .fullcov_vae import synthetic_data


class Variational(BayesianNet):
    def __init__(self, x_dim, z_dim, hidden, n_samples):
        super().__init__()
        self.n_samples = n_samples
        self.body = nn.Sequential(nn.Linear(x_dim, hidden), nn.ReLU())
        self.mean_head = nn.Linear(hidden, z_dim)
        self.logstd_head = nn.Linear(hidden, z_dim)

    def encode(self, x):
        h = self.body(x)
        return self.mean_head(h), self.logstd_head(h)

    def forward(self, observed):
        self.observe(observed)
        mean, logstd = self.encode(self.observed['x'])
        self.normal('z', mean=mean, logstd=logstd, n_samples=self.n_samples, group_ndims=1)
        return self


class Generator(BayesianNet):
    """``encode``: the variational net's encoder (shared, not owned: held in a list so that it is registered once)."""

    def __init__(self, x_dim, z_dim, hidden, n_samples, n_components, encode):
        super().__init__()
        self.z_dim, self.n_samples, self._encode = z_dim, n_samples, [encode]
        self.pseudo_inputs = nn.Parameter(torch.rand(n_components, x_dim))
        self.dec = nn.Sequential(nn.Linear(z_dim, hidden), nn.ReLU(), nn.Linear(hidden, x_dim))

    def prior(self):
        """(logits [C], mean [C, D], logstd [C, D]) of the VampPrior"""
        mean, logstd = self._encode[0](torch.sigmoid(self.pseudo_inputs))
        return torch.zeros(mean.shape[0], dtype=mean.dtype, device=mean.device), mean, logstd

    def forward(self, observed):
        self.observe(observed)
        batch = self.observed['z'].shape[-2] if 'z' in self.observed else 16
        logits, mean, logstd = self.prior()
        z = self.normal_mixture('z', logits, mean, logstd=logstd, batch_shape=(batch,), n_samples=self.n_samples)
        self.bernoulli('x', logits=self.dec(z), group_ndims=1)
        return self


def build(k=1, x_dim=64, z_dim=8, hidden=64, n_components=50, device='cuda'):
    """The objective: the ELBO for k == 1, the importance-weighted bound over k particles otherwise (both 'sgvb')."""
    K = int(k) if int(k) > 1 else None
    var = Variational(x_dim, z_dim, hidden, K)
    gen = Generator(x_dim, z_dim, hidden, K, n_components, var.encode)
    if K is None:
        return ELBO(gen, var, estimator='sgvb').to(device)
    return ImportanceWeightedObjective(gen, var, axis=0, estimator='sgvb').to(device)


def main(k=1, steps=200, batch=32, lr=3e-3, seed=0, device='cuda', log_every=50, **sizes):
    """Train; returns (the bound per step, the objective)."""
    torch.manual_seed(seed)
    device = torch.device(device)
    model = build(k, device=device, **sizes)
    opt = torch.optim.Adam(model.parameters(), lr)
    x_all = synthetic_data(batch * 8, sizes.get('x_dim', 64), seed=seed).to(device)
    bounds = []
    for step in range(steps):
        i = (step % 8) * batch
        loss = model({'x': x_all[i:i + batch]})
        opt.zero_grad()
        loss.backward()
        opt.step()
        bounds.append(-float(loss.detach()))
        if log_every and (step + 1) % log_every == 0:
            print("k=%d step %d  bound %.4f" % (k, step + 1, bounds[-1]))
    return bounds, model


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--k', type=int, default=1, help="particles: 1 trains the ELBO, more the importance-weighted bound")
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--components', type=int, default=50)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    b, _ = main(args.k, steps=args.steps, batch=args.batch, seed=args.seed, n_components=args.components)
    print("k=%d: first 10 steps %.4f, last 10 steps %.4f" % (args.k, sum(b[:10]) / 10, sum(b[-10:]) / 10))
