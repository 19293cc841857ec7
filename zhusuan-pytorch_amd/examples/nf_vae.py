"""VAE whose posterior sample goes through a planar or a Householder flow of the package: ``zhusuan.transform`` on the fused
kernels of include/zs_nf.h, the whole stack of layers one launch.

The generator and the variational net are those of ``examples.flow_vae`` (the reference caller
examples/normlizing_flows/flow_vae.py), and so are ``train`` and the command line; the two transforms that file spells out as
plain torch modules are ``zhusuan.transform.PlanarFlow`` and ``zhusuan.transform.HouseholderFlow`` here, which also lets the
planar stack be deeper than one layer (``--n-planar``)."""
import argparse
import time

import torch

from zhusuan.transform import PlanarFlow, HouseholderFlow
from zhusuan.variational.elbo import ELBO

from examples import vae_mnist
from examples.flow_vae import Variational, train


def build(method="Planar", batch_size=64, x_dim=784, z_dim=40, hidden=500, device='cuda', n_planar=1, n_householder=5):
    """The reference's sizes by default (flow_vae.py:179-201).  ``method``: "Planar" | "HouseHolder"."""
    generator = vae_mnist.Generator(x_dim, z_dim, batch_size, hidden)
    variational = Variational(x_dim, z_dim, batch_size, hidden)
    if method == "Planar":
        model = ELBO(generator, variational, transform=PlanarFlow(z_dim, n_planar, name='z'), transform_var=['z'])
    elif method == "HouseHolder":
        flow = HouseholderFlow(z_dim, hidden, n_householder, name='z')
        model = ELBO(generator, variational, transform=flow, transform_var=['z'], auxillary_var=['z_logits'])
    else:
        raise NotImplementedError("please select correct method")
    return model.to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--method', default='Planar', choices=['Planar', 'HouseHolder'])
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--n-planar', type=int, default=1)
    ap.add_argument('--n-householder', type=int, default=5)
    args = ap.parse_args()
    device = torch.device('cuda')
    model = build(args.method, args.batch, device=device, n_planar=args.n_planar, n_householder=args.n_householder)
    g = torch.Generator().manual_seed(1234)
    x_all = (torch.rand(args.batch * 32, 784, generator=g) < 0.5).float().to(device)
    t0 = time.time()
    train(model, x_all, args.batch, args.steps, log=print)
    torch.cuda.synchronize()
    print("%.1f ELBO-evals/s" % (args.batch * args.steps / (time.time() - t0)))


if __name__ == '__main__':
    main()
