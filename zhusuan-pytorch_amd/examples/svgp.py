"""A sparse variational Gaussian process (upstream ZhuSuan's examples/gaussian_process/svgp.py) on synthetic regression data.

q(f_Z) = MultivariateNormalCholesky(mean [M], tril [M, M]) over the values at M inducing inputs; f | f_Z = GPConditional at the
batch's inputs, in the model and in the variational alike, as upstream writes it; y ~ Normal(f, noise).  (The objectives of this
package re-draw every latent of the variational net after it has run, as the reference does: f is drawn around the conditional
mean of the first draw of f_Z and scored in the model under the second, so the two conditional densities differ by the distance
of the two means and do not cancel exactly.)
The conditional's moments and their gradients run on the kernels of include/zs_gp.h (``zhusuan.explain(node.dist)`` names them);
the package has no CPU path for the other nodes, so the example needs a HIP device.  Trained by the reparameterised ELBO with
FlatAdam.

    python examples/svgp.py [--steps 200] [--inducing 32] [--dim 1] [--particles 10]"""
import argparse

import torch

import zhusuan as zs
from zhusuan.distributions import GPConditional
from zhusuan.framework.bn import BayesianNet
from zhusuan.optim import FlatAdam
from zhusuan.variational.elbo import ELBO


class Net(BayesianNet):
    def __init__(self, build):
        super().__init__()
        self.build = build

    def forward(self, observed):
        self.observe(observed)
        self.build(self)
        return self


def init_params(x, n_inducing, generator, dtype=torch.float32):
    """inducing inputs at a random subset of x, unit lengthscales and amplitude, q(f_Z) = N(0, I), noise 0.3"""
    n, d = x.shape
    pick = torch.randperm(n, generator=generator)[:n_inducing]
    return dict(inducing=x[pick].clone().to(dtype), log_length=torch.zeros(d, dtype=dtype), log_amp=torch.zeros((), dtype=dtype),
                q_mean=torch.zeros(n_inducing, dtype=dtype), q_raw=torch.eye(n_inducing, dtype=dtype),
                log_noise=torch.tensor(-1.2, dtype=dtype))


def q_tril(raw):
    """a lower-triangular factor with a positive diagonal from an unconstrained matrix"""
    return torch.tril(raw, -1) + torch.diag_embed(torch.abs(torch.diagonal(raw)) + 1e-3)


def build(params, x, particles=10, jitter=1e-2, device=torch.device("cuda:0")):
    """The ELBO of the sparse GP over the inputs x [N, d]; the jitter is relative to amplitude^2."""
    m = params['inducing'].shape[0]
    n = x.shape[0]

    step = {}          # the kernel's quantities of the current step: the variational net runs first and the model reuses them

    def q(net):
        length, amp = torch.exp(params['log_length']), torch.exp(params['log_amp'])
        step['kernel'] = length, amp, GPConditional.gram_tril(params['inducing'], length, amp, jitter=jitter * amp ** 2)
        fz = net.multivariate_normal_cholesky('fz', params['q_mean'], q_tril(params['q_raw']), n_samples=particles)
        net.gp_conditional('f', x, params['inducing'], fz, step['kernel'][2], length, amp, group_ndims=1)

    def p(net):
        length, amp, tril = step['kernel']
        fz = net.multivariate_normal_cholesky('fz', torch.zeros(m, dtype=x.dtype, device=device), tril, n_samples=particles)
        f = net.gp_conditional('f', x, params['inducing'], fz, tril, length, amp, group_ndims=1)
        net.normal('y', mean=f, std=torch.exp(params['log_noise']) * torch.ones(n, dtype=x.dtype, device=device), group_ndims=1)
    return ELBO(Net(p).to(device), Net(q).to(device), estimator="sgvb").to(device)


def synthetic(n, d, generator):
    x = 3.0 * torch.rand(n, d, generator=generator) - 1.5
    return x, torch.sin(2.0 * x.sum(-1)) + 0.3 * torch.randn(n, generator=generator)


def main(steps=200, n_data=512, dim=1, inducing=32, particles=10, lr=2e-2, device="cuda:0", log_every=50, seed=0):
    """Trains and returns (the losses, the parameters, the objective)."""
    device = torch.device(device)
    torch.cuda.manual_seed(seed)          # the device's Philox streams: the run is reproducible
    g = torch.Generator().manual_seed(seed)
    x, y = synthetic(n_data, dim, g)
    params = {k: v.to(device).requires_grad_(True) for k, v in init_params(x, inducing, g).items()}
    x, y = x.to(device), y.to(device)
    objective = build(params, x, particles=particles, device=device)
    opt = FlatAdam(list(params.values()), lr=lr)
    losses = []
    for step in range(steps):
        opt.zero_grad()
        loss = objective({'y': y})
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        if log_every and (step % log_every == 0 or step == steps - 1):
            print("step %4d  -ELBO %.3f" % (step, losses[-1]))
    if log_every:
        print("conditional: %s" % zs.explain(objective.variational.nodes['f'].dist))
    return losses, params, objective


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--inducing", type=int, default=32)
    ap.add_argument("--dim", type=int, default=1)
    ap.add_argument("--particles", type=int, default=10)
    a = ap.parse_args()
    main(steps=a.steps, dim=a.dim, inducing=a.inducing, particles=a.particles)
