"""A VAE / IWAE with a full-covariance Gaussian posterior on synthetic binarised data: the encoder emits a mean and the
D (D + 1) / 2 entries of the Cholesky factor L of the posterior covariance (the diagonal through ``exp``, assembled in torch), the
latent is a ``multivariate_normal_cholesky`` node, the prior a standard ``normal`` over the given draw.  Trained two ways through
the objectives as they stand:

    k == 1   ELBO(estimator='sgvb')
    k  > 1   ImportanceWeightedObjective(axis=0, estimator='sgvb') with k particles

The latent's draw with its log-density is one launch (V1 of include/zs_mvn.h), its gradient one more.
"""
import argparse

import torch
import torch.nn as nn

from zhusuan.framework.bn import BayesianNet
from zhusuan.variational.elbo import ELBO
from zhusuan.variational.importance_weighted_objective import ImportanceWeightedObjective


def assemble_tril(flat, n_dims):
    """``[..., D (D + 1) / 2]`` -> lower-triangular ``[..., D, D]``: the entries row by row, the diagonal through ``exp``."""
    rows, cols = torch.tril_indices(n_dims, n_dims, device=flat.device)
    scatter = torch.zeros(flat.shape[-1], n_dims * n_dims, dtype=flat.dtype, device=flat.device)
    scatter[torch.arange(flat.shape[-1], device=flat.device), rows * n_dims + cols] = 1
    L = (flat @ scatter).reshape(tuple(flat.shape[:-1]) + (n_dims, n_dims))
    diag = torch.diagonal(L, dim1=-2, dim2=-1)
    return L - torch.diag_embed(diag) + torch.diag_embed(torch.exp(diag))


class Generator(BayesianNet):
    def __init__(self, x_dim, z_dim, hidden, n_samples):
        super().__init__()
        self.z_dim, self.n_samples = z_dim, n_samples
        self.dec = nn.Sequential(nn.Linear(z_dim, hidden), nn.ReLU(), nn.Linear(hidden, x_dim))

    def forward(self, observed):
        self.observe(observed)
        batch = self.observed['z'].shape[-2] if 'z' in self.observed else 16
        zeros = torch.zeros(batch, self.z_dim, device=self.device)
        z = self.normal('z', mean=zeros, std=torch.ones_like(zeros), n_samples=self.n_samples, group_ndims=1)
        self.bernoulli('x', logits=self.dec(z), group_ndims=1)
        return self


class Variational(BayesianNet):
    def __init__(self, x_dim, z_dim, hidden, n_samples):
        super().__init__()
        self.z_dim, self.n_samples = z_dim, n_samples
        self.body = nn.Sequential(nn.Linear(x_dim, hidden), nn.ReLU())
        self.mean_head = nn.Linear(hidden, z_dim)
        self.tril_head = nn.Linear(hidden, z_dim * (z_dim + 1) // 2)

    def forward(self, observed):
        self.observe(observed)
        h = self.body(self.observed['x'])
        self.multivariate_normal_cholesky('z', self.mean_head(h), assemble_tril(0.1 * self.tril_head(h), self.z_dim),
                                          n_samples=self.n_samples)
        return self


def build(k=1, x_dim=64, z_dim=8, hidden=64, device='cuda'):
    """The objective: the ELBO for k == 1, the importance-weighted bound over k particles otherwise (both 'sgvb')."""
    K = int(k) if int(k) > 1 else None
    gen, var = Generator(x_dim, z_dim, hidden, K), Variational(x_dim, z_dim, hidden, K)
    if K is None:
        return ELBO(gen, var, estimator='sgvb').to(device)
    return ImportanceWeightedObjective(gen, var, axis=0, estimator='sgvb').to(device)


def synthetic_data(n, x_dim=64, n_prototypes=8, flip=0.1, seed=0):
    """n binarised rows: one of `n_prototypes` random bit patterns with every bit flipped with probability `flip`."""
    g = torch.Generator().manual_seed(seed)
    protos = (torch.rand(n_prototypes, x_dim, generator=g) < 0.5).float()
    which = torch.randint(0, n_prototypes, (n,), generator=g)
    noise = (torch.rand(n, x_dim, generator=g) < flip).float()
    return (protos[which] - noise).abs()


def main(k=1, steps=200, batch=32, lr=3e-3, seed=0, device='cuda', log_every=50, **sizes):
    """Train; returns the bound per step (minus the loss)."""
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
    return bounds


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--k', type=int, default=1, help="particles: 1 trains the ELBO, more the importance-weighted bound")
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    b = main(args.k, steps=args.steps, batch=args.batch, seed=args.seed)
    print("k=%d: first 10 steps %.4f, last 10 steps %.4f" % (args.k, sum(b[:10]) / 10, sum(b[-10:]) / 10))
