"""VAE whose posterior sample goes through a normalising flow before the decoder: ``ELBO(transform=...)``.

Counterpart of the reference caller examples/normlizing_flows/flow_vae.py:18-249, on synthetic data: the same generator and
variational nets (``examples.vae_mnist``'s, plus the ``z_logits`` cache entry the Householder variant reads) and the three
transforms -- ``NICEFlow`` (ten ``MaskCoupling`` layers and a ``Scaling``: the layers of ``zhusuan.invertible``, on the kernels
of include/zs_flow.h), ``PlanarFlow`` and ``HouseHolderFlow`` (plain torch modules, as in the reference; the latter takes the
auxiliary variable ``z_logits``)."""
import argparse
import time

import torch
import torch.nn as nn
import torch.nn.functional as F

from zhusuan.variational.elbo import ELBO
from zhusuan.invertible import MaskCoupling, get_coupling_mask, Scaling, RevSequential, RevNet

from examples import vae_mnist


class Variational(vae_mnist.Variational):
    def forward(self, observed):
        self.observe(observed)
        x = self.observed['x']
        z_logits = self.sq(x)
        self.cache['z_logits'] = z_logits
        z_mean = self.fc3(z_logits)
        z_std = torch.exp(self.fc4(z_logits))
        self.normal(name='z', mean=z_mean, std=z_std, reduce_mean_dims=[0], reduce_sum_dims=[1])
        return self


class NICEFlow(nn.Module):
    def __init__(self, z_dim, mid_dim, num_coupling, num_hidden, device='cuda'):
        super(NICEFlow, self).__init__()
        masks = get_coupling_mask(z_dim, 1, num_coupling)
        flows = [MaskCoupling(in_out_dim=z_dim, mid_dim=mid_dim, hidden=num_hidden, mask=masks[i].to(device))
                 for i in range(num_coupling)]
        flows.append(Scaling(z_dim))
        self.flow = RevSequential(flows)

    def forward(self, z, **kwargs):
        out, log_det_J = self.flow.forward(z[0], **kwargs)
        return {"z": out}, log_det_J


class PF(nn.Module):
    """One planar flow ``z' = z + u_hat tanh(w.z + b)`` (Rezende & Mohamed 2015).  ``u_hat`` is ``u`` with its component along
    ``w`` moved so that ``w.u_hat = softplus(w.u) - 1 > -1``, which keeps the map invertible; the Jacobian determinant is
    ``1 + (1 - tanh^2(w.z + b)) w.u_hat``."""

    def __init__(self, z_dim):
        super(PF, self).__init__()
        self.u, self.w, self.b = (nn.Parameter(torch.rand(shape)) for shape in ([1, z_dim], [1, z_dim], [1]))

    def forward(self, z, **kwargs):
        wu = (self.w * self.u).sum()
        w_unit_sq = self.w / (self.w * self.w).sum()
        u_hat = self.u + (F.softplus(wu) - 1. - wu) * w_unit_sq
        t = torch.tanh(z @ self.w.t() + self.b)                       # [B, 1]
        slope = (1. - t * t) * (self.w * u_hat).sum()                 # (1 - tanh^2) w.u_hat, [B, 1]
        return z + u_hat * t, torch.log(torch.abs(1. + slope))


class PlanarFlow(nn.Module):
    def __init__(self, z_dim, n_flows):
        super(PlanarFlow, self).__init__()
        self.flows = nn.Sequential(*[PF(z_dim) for _ in range(n_flows)])

    def forward(self, z, **kwargs):
        out, log_det = self.flows(z[0])
        return {'z': out}, log_det


class HF(RevNet):
    """One Householder reflection ``z' = z - 2 v (v.z) / |v|^2`` (Tomczak & Welling 2016) about a vector ``v`` computed from
    the previous one (the first from the auxiliary variable); a reflection preserves volume, so the log-det is zero."""

    def __init__(self, z_dim, is_first=False, v_dim=None):
        super(HF, self).__init__()
        self.v_layer = nn.Linear(v_dim if is_first else z_dim, z_dim)

    def _forward(self, inputs, **kwargs):
        z, v_prev = inputs[0], inputs[1]
        v = self.v_layer(v_prev)
        along = (v * z).sum(1, keepdim=True) / (v * v).sum(1, keepdim=True)
        return (z - 2. * along * v, v), torch.zeros([1, 1], device=z.device)


class HouseHolderFlow(RevNet):
    def __init__(self, z_dim, v_dim, n_flows):
        super(HouseHolderFlow, self).__init__()
        self.flow = RevSequential([HF(z_dim, is_first=True, v_dim=v_dim) if i == 0 else HF(z_dim) for i in range(n_flows)])

    def _forward(self, inputs, **kwargs):
        out, log_det = self.flow.forward(inputs, **kwargs)
        return {"z": out[0]}, log_det


def build(method="NICE", batch_size=64, x_dim=784, z_dim=40, hidden=500, device='cuda', mid_dim_flow=64, num_coupling=10,
          num_hidden_per_coupling=4, n_planar=1, n_householder=5):
    """The reference's sizes by default (flow_vae.py:179-201).  ``method``: "NICE" | "Planar" | "HouseHolder"."""
    generator = vae_mnist.Generator(x_dim, z_dim, batch_size, hidden)
    variational = Variational(x_dim, z_dim, batch_size, hidden)
    if method == "NICE":
        flow = NICEFlow(z_dim, mid_dim_flow, num_coupling, num_hidden_per_coupling, device=device)
        model = ELBO(generator, variational, transform=flow, transform_var=['z'])
    elif method == "Planar":
        model = ELBO(generator, variational, transform=PlanarFlow(z_dim, n_planar), transform_var=['z'])
    elif method == "HouseHolder":
        flow = HouseHolderFlow(z_dim, hidden, n_householder)
        model = ELBO(generator, variational, transform=flow, transform_var=['z'], auxillary_var=['z_logits'])
    else:
        raise NotImplementedError("please select correct method")
    return model.to(device)


def train(model, x_all, batch, steps, lr=1e-3, log=None):
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    n_batches = max(x_all.shape[0] // batch, 1)
    losses = []
    for step in range(steps):
        i = (step % n_batches) * batch
        loss = model({'x': x_all[i:i + batch]})
        loss.backward()
        opt.step()
        opt.zero_grad()
        losses.append(float(loss.detach()))
        if log and (step + 1) % 50 == 0:
            log("step %d  loss %.4f" % (step + 1, losses[-1]))
    return losses


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--method', default='NICE', choices=['NICE', 'Planar', 'HouseHolder'])
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--steps', type=int, default=200)
    args = ap.parse_args()
    device = torch.device('cuda')
    model = build(args.method, args.batch, device=device)
    g = torch.Generator().manual_seed(1234)
    x_all = (torch.rand(args.batch * 32, 784, generator=g) < 0.5).float().to(device)
    t0 = time.time()
    train(model, x_all, args.batch, args.steps, log=print)
    torch.cuda.synchronize()
    print("%.1f ELBO-evals/s" % (args.batch * args.steps / (time.time() - t0)))


if __name__ == '__main__':
    main()
