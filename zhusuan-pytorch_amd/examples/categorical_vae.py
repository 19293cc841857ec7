"""A VAE with D categorical latents of N categories each on synthetic binarised data, trained three ways through the
objectives as they stand:

    'vimco'      ImportanceWeightedObjective(axis=0, estimator='vimco') over an ``onehot_categorical`` latent, K particles
    'reinforce'  ELBO(estimator='reinforce') over the same latent
    'sgvb'       ELBO(estimator='sgvb') over the relaxed ``exp_concrete`` latent (the decoder is fed exp(y))

The latent's draw with its log-mass / log-density is one launch (C1 / C3 of include/zs_cat.h), its gradient one more.
"""
import argparse

import torch
import torch.nn as nn

from zhusuan.framework.bn import BayesianNet
from zhusuan.variational.elbo import ELBO
from zhusuan.variational.importance_weighted_objective import ImportanceWeightedObjective


class Generator(BayesianNet):
    def __init__(self, x_dim, n_latents, n_categories, hidden, relaxed, temperature, n_samples):
        super().__init__()
        self.D, self.N = n_latents, n_categories
        self.relaxed, self.temperature, self.n_samples = relaxed, temperature, n_samples
        self.dec = nn.Sequential(nn.Linear(n_latents * n_categories, hidden), nn.ReLU(), nn.Linear(hidden, x_dim))

    def forward(self, observed):
        self.observe(observed)
        batch = self.observed['z'].shape[-3] if 'z' in self.observed else 16
        prior = torch.zeros(batch, self.D, self.N, device=self.device)
        if self.relaxed:
            y = self.exp_concrete('z', self.temperature, prior, n_samples=self.n_samples, group_ndims=1)
            z = torch.exp(y)
        else:
            z = self.onehot_categorical('z', prior, n_samples=self.n_samples, group_ndims=1)
        logits = self.dec(z.reshape(tuple(z.shape[:-2]) + (self.D * self.N,)))
        self.cache['x_logits'] = logits
        self.bernoulli('x', logits=logits, group_ndims=1)
        return self


class Variational(BayesianNet):
    def __init__(self, x_dim, n_latents, n_categories, hidden, relaxed, temperature, n_samples):
        super().__init__()
        self.D, self.N = n_latents, n_categories
        self.relaxed, self.temperature, self.n_samples = relaxed, temperature, n_samples
        self.enc = nn.Sequential(nn.Linear(x_dim, hidden), nn.ReLU(), nn.Linear(hidden, n_latents * n_categories))

    def forward(self, observed):
        self.observe(observed)
        x = self.observed['x']
        logits = self.enc(x).reshape(x.shape[0], self.D, self.N)
        if self.relaxed:
            self.exp_concrete('z', self.temperature, logits, n_samples=self.n_samples, group_ndims=1)
        else:
            self.onehot_categorical('z', logits, n_samples=self.n_samples, group_ndims=1)
        return self


def build(mode='vimco', x_dim=64, n_latents=4, n_categories=8, hidden=64, n_samples=8, temperature=0.67, device='cuda'):
    """The objective of one of the three ways (see the module docstring)."""
    if mode not in ('vimco', 'reinforce', 'sgvb'):
        raise ValueError("mode: 'vimco', 'reinforce' or 'sgvb'")
    relaxed = mode == 'sgvb'
    K = n_samples if mode == 'vimco' else None
    gen = Generator(x_dim, n_latents, n_categories, hidden, relaxed, temperature, K)
    var = Variational(x_dim, n_latents, n_categories, hidden, relaxed, temperature, K)
    if mode == 'vimco':
        return ImportanceWeightedObjective(gen, var, axis=0, estimator='vimco').to(device)
    return ELBO(gen, var, estimator='reinforce' if mode == 'reinforce' else 'sgvb').to(device)


def synthetic_data(n, x_dim=64, n_prototypes=8, flip=0.1, seed=0):
    """n binarised rows: one of `n_prototypes` random bit patterns with every bit flipped with probability `flip`."""
    g = torch.Generator().manual_seed(seed)
    protos = (torch.rand(n_prototypes, x_dim, generator=g) < 0.5).float()
    which = torch.randint(0, n_prototypes, (n,), generator=g)
    noise = (torch.rand(n, x_dim, generator=g) < flip).float()
    return (protos[which] - noise).abs()


def main(mode='vimco', steps=200, batch=32, lr=3e-3, seed=0, device='cuda', log_every=50, **sizes):
    """Train one way; returns the bound per step (the importance-weighted bound for 'vimco', minus the loss otherwise)."""
    torch.manual_seed(seed)
    device = torch.device(device)
    x_dim = sizes.get('x_dim', 64)
    model = build(mode, device=device, **sizes)
    opt = torch.optim.Adam(model.parameters(), lr)
    x_all = synthetic_data(batch * 8, x_dim, seed=seed).to(device)
    bounds = []
    for step in range(steps):
        i = (step % 8) * batch
        loss = model({'x': x_all[i:i + batch]})
        opt.zero_grad()
        loss.backward()
        opt.step()
        bounds.append(float(model.last_iw_bound.mean()) if mode == 'vimco' else -float(loss.detach()))
        if log_every and (step + 1) % log_every == 0:
            print("%s step %d  bound %.4f" % (mode, step + 1, bounds[-1]))
    return bounds


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', default='all', choices=['all', 'vimco', 'reinforce', 'sgvb'])
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    for m in (['vimco', 'reinforce', 'sgvb'] if args.mode == 'all' else [args.mode]):
        b = main(m, steps=args.steps, batch=args.batch, seed=args.seed)
        print("%s: first 10 steps %.4f, last 10 steps %.4f" % (m, sum(b[:10]) / 10, sum(b[-10:]) / 10))
