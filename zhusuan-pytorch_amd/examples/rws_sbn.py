"""A sigmoid belief network on synthetic binarised data, trained by reweighted wake-sleep (Bornschein & Bengio 2015):

    latent 'bernoulli'   two Bernoulli layers   h2 -> h1 -> x   with the recognition net   x -> h1 -> h2
    latent 'onehot'      one layer of D one-hot variables of N categories   z -> x,   x -> z

    estimator 'rws'      InclusiveKLObjective(axis=0, model_grad=True): wake-wake, one backward trains both nets with the
                         self-normalised importance weights of K particles; ``sleep=True`` adds the sleep phase
                         (``sleep_cost``: q's log-probability of the generator's dreams)
    estimator 'vimco'    ImportanceWeightedObjective(axis=0, estimator='vimco') over the same nets, for comparison

The weights, the cost, the bound and the effective sample size are one launch (Q1 of include/zs_klpq.h), the gradient of every
node's log-probability one more.  The figure reported is the importance-sampled log-likelihood ``zhusuan.is_loglikelihood`` with
the same K particles.
"""
import argparse

import torch
import torch.nn as nn

import zhusuan as zs
from zhusuan.framework.bn import BayesianNet
from zhusuan.variational import ImportanceWeightedObjective, InclusiveKLObjective


class Generator(BayesianNet):
    def __init__(self, latent, x_dim, h1, h2, n_latents, n_categories, n_samples, batch):
        super().__init__()
        self.latent, self.n_samples, self.batch = latent, n_samples, batch
        self.D, self.N = n_latents, n_categories
        if latent == 'bernoulli':
            self.prior = nn.Parameter(torch.zeros(h2))
            self.dec2 = nn.Linear(h2, h1)
            self.dec1 = nn.Linear(h1, x_dim)
        else:
            self.prior = nn.Parameter(torch.zeros(n_latents, n_categories))
            self.dec1 = nn.Linear(n_latents * n_categories, x_dim)

    def forward(self, observed):
        self.observe(observed)
        top = 'h2' if self.latent == 'bernoulli' else 'z'
        rows = self.prior.dim() + 1          # the batch axis of the top latent, counted from the end
        batch = self.observed[top].shape[-rows] if top in self.observed else self.batch
        prior = self.prior.expand((batch,) + tuple(self.prior.shape))
        if self.latent == 'bernoulli':
            h2 = self.bernoulli('h2', logits=prior, n_samples=self.n_samples, group_ndims=1)
            h1 = self.bernoulli('h1', logits=self.dec2(h2), group_ndims=1)
        else:
            z = self.onehot_categorical('z', prior, n_samples=self.n_samples, group_ndims=1)
            h1 = z.reshape(tuple(z.shape[:-2]) + (self.D * self.N,))
        self.bernoulli('x', logits=self.dec1(h1), group_ndims=1)
        return self


class Variational(BayesianNet):
    def __init__(self, latent, x_dim, h1, h2, n_latents, n_categories, n_samples):
        super().__init__()
        self.latent, self.n_samples = latent, n_samples
        self.D, self.N = n_latents, n_categories
        if latent == 'bernoulli':
            self.enc1 = nn.Linear(x_dim, h1)
            self.enc2 = nn.Linear(h1, h2)
        else:
            self.enc1 = nn.Linear(x_dim, n_latents * n_categories)

    def forward(self, observed):
        self.observe(observed)
        x = self.observed['x']
        # a value with the particle axis already in it (a dream of K particles) needs no further particles
        n = self.n_samples if x.dim() == 2 else None
        if self.latent == 'bernoulli':
            h1 = self.bernoulli('h1', logits=self.enc1(x), n_samples=n, group_ndims=1)
            self.bernoulli('h2', logits=self.enc2(h1), group_ndims=1)
        else:
            logits = self.enc1(x)
            self.onehot_categorical('z', logits.reshape(tuple(logits.shape[:-1]) + (self.D, self.N)), n_samples=n, group_ndims=1)
        return self


def build(estimator='rws', latent='bernoulli', x_dim=64, h1=32, h2=16, n_latents=4, n_categories=8, n_samples=8, batch=32,
          device='cuda'):
    """The objective over a fresh pair of nets (see the module docstring)."""
    if estimator not in ('rws', 'vimco') or latent not in ('bernoulli', 'onehot'):
        raise ValueError("estimator: 'rws' or 'vimco'; latent: 'bernoulli' or 'onehot'")
    gen = Generator(latent, x_dim, h1, h2, n_latents, n_categories, n_samples, batch)
    var = Variational(latent, x_dim, h1, h2, n_latents, n_categories, n_samples)
    if estimator == 'vimco':
        return ImportanceWeightedObjective(gen, var, axis=0, estimator='vimco').to(device)
    return InclusiveKLObjective(gen, var, axis=0, estimator='rws', model_grad=True).to(device)


def synthetic_data(n, x_dim=64, n_prototypes=8, flip=0.1, seed=0):
    """n binarised rows: one of `n_prototypes` random bit patterns with every bit flipped with probability `flip`."""
    g = torch.Generator().manual_seed(seed)
    protos = (torch.rand(n_prototypes, x_dim, generator=g) < 0.5).float()
    which = torch.randint(0, n_prototypes, (n,), generator=g)
    noise = (torch.rand(n, x_dim, generator=g) < flip).float()
    return (protos[which] - noise).abs()


def main(estimator='rws', latent='bernoulli', sleep=False, steps=200, batch=32, lr=3e-3, seed=0, device='cuda', log_every=50,
         **sizes):
    """Train; returns the mean importance-sampled log-likelihood of each step's batch, taken before that step's update."""
    torch.manual_seed(seed)
    device = torch.device(device)
    x_dim = sizes.get('x_dim', 64)
    model = build(estimator, latent, batch=batch, device=device, **sizes)
    opt = torch.optim.Adam(model.parameters(), lr)
    x_all = synthetic_data(batch * 8, x_dim, seed=seed).to(device)
    history = []
    for step in range(steps):
        i = (step % 8) * batch
        x = x_all[i:i + batch]
        history.append(float(zs.is_loglikelihood(model.generator, model.variational, {'x': x}, axis=0).mean()))
        loss = model({'x': x})
        if sleep and estimator == 'rws':
            loss = loss + model.sleep_cost(['x'], n_samples=model.generator.n_samples)
        opt.zero_grad()
        loss.backward()
        opt.step()
        if log_every and (step + 1) % log_every == 0:
            print("%s/%s step %d  log-likelihood %.4f" % (estimator, latent, step + 1, history[-1]))
    return history


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--estimator', default='rws', choices=['rws', 'vimco'])
    ap.add_argument('--latent', default='bernoulli', choices=['bernoulli', 'onehot'])
    ap.add_argument('--sleep', action='store_true', help="add the sleep phase to the wake-wake update (rws only)")
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    h = main(args.estimator, args.latent, sleep=args.sleep, steps=args.steps, batch=args.batch, seed=args.seed)
    print("%s/%s: importance-sampled log-likelihood, first 10 steps %.4f, last 10 steps %.4f"
          % (args.estimator, args.latent, sum(h[:10]) / 10, sum(h[-10:]) / 10))
