"""Shared by the flow golden tests and by tests/golden/flow/gen_flow_golden.py (a helper, not a test): the small layers and
models of the fixtures, written once against the ``zhusuan.invertible`` / ``BayesianNet`` / ``ELBO`` interfaces, so that the
generator builds them on the reference's classes and the tests on this package's.  Weights are not re-derived from a seed by
the tests: the generator stores every ``state_dict`` in the fixture."""
import numpy as np
import torch
import torch.nn as nn

B, D, H = 4, 6, 8
X_DIM, Z_DIM = 6, 5
LAYERS = ["maskcoupling", "coupling", "scaling", "made", "sequential"]
SEEDS = {"maskcoupling": 21, "coupling": 22, "scaling": 23, "made": 24, "sequential": 25, "nice": 26, "elbo": 27}
LD_WEIGHT = 0.7          # loss of a layer case: sum(y * gy) + LD_WEIGHT * sum(log_det)


def make_layer(inv, kind):
    """``inv``: the module ``zhusuan.invertible`` (the reference's or this package's)."""
    masks = inv.get_coupling_mask(D, 1, 2)
    if kind == "maskcoupling":
        return inv.MaskCoupling(D, H, 2, masks[0])
    if kind == "coupling":
        return inv.Coupling(D, H, 2, 1)
    if kind == "scaling":
        return inv.Scaling(D)
    if kind == "made":
        return inv.MADE(D, H, 2)
    if kind == "sequential":
        return inv.RevSequential([inv.MaskCoupling(D, H, 2, masks[0]), inv.Coupling(D, H, 1, 0), inv.MaskCoupling(D, H, 1, masks[1]),
                                  inv.Scaling(D)])
    raise ValueError(kind)


def randomize(module, seed):
    """Seeded N(0, 0.5^2) values for every parameter (the constructors' zeros of Scaling.log_scale would test nothing)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_((0.5 * torch.randn(p.shape, generator=g, dtype=torch.float64)).to(p.dtype))
    return module


def layer_data(kind):
    rng = np.random.RandomState(SEEDS[kind])
    return rng.standard_normal((B, D)).astype(np.float32), rng.standard_normal((B, D)).astype(np.float32)


def make_nice(inv, dists, BayesianNet, dtype=torch.float32, device=torch.device("cpu")):
    """examples/normlizing_flows/nice_mnist.py:13-38 of the reference at D = 6: three couplings and a scaling."""
    class NICE(BayesianNet):
        def __init__(self):
            super().__init__()
            masks = inv.get_coupling_mask(D, 1, 3)
            self.flow = inv.RevSequential([inv.MaskCoupling(D, H, 2, masks[i].to(device)) for i in range(3)] + [inv.Scaling(D)])
            dis = dists.Logistic(loc=torch.zeros([D], dtype=dtype, device=device), scale=torch.ones([D], dtype=dtype, device=device))
            self.sn(dists.FlowDistribution(latents=dis, transformation=self.flow, dtype=dtype), name="x", n_samples=-1)

        def forward(self, x):
            return self.nodes['x'].log_prob(x)
    return NICE()


def make_elbo(inv, dists, BayesianNet, ELBO, dtype=torch.float32, device=torch.device("cpu")):
    """examples/normlizing_flows/flow_vae.py:18-103 of the reference at B = 4, x = 6, z = 5 with its NICE transform."""
    class Generator(BayesianNet):
        def __init__(self):
            super().__init__()
            self.gen = nn.Sequential(nn.Linear(Z_DIM, H), nn.ReLU(), nn.Linear(H, X_DIM), nn.Sigmoid())

        def forward(self, observed):
            self.observe(observed)
            n = self.observed['z'].shape[0]
            prior = dists.Normal(mean=torch.zeros([n, Z_DIM], dtype=dtype, device=device),
                                 std=torch.ones([n, Z_DIM], dtype=dtype, device=device))
            z = self.sn(prior, "z", reduce_mean_dims=[0], reduce_sum_dims=[1])
            self.sn(dists.Bernoulli(probs=self.gen(z)), "x", reduce_mean_dims=[0], reduce_sum_dims=[1])
            return self

    class Variational(BayesianNet):
        def __init__(self):
            super().__init__()
            self.common = nn.Sequential(nn.Linear(X_DIM, H), nn.ReLU())
            self.output_mean = nn.Linear(H, Z_DIM)
            self.output_sd = nn.Linear(H, Z_DIM)

        def forward(self, observed):
            self.observe(observed)
            h = self.common(self.observed['x'])
            normal = dists.Normal(mean=self.output_mean(h), std=torch.exp(self.output_sd(h)), is_reparameterized=True)
            self.sn(normal, "z", reduce_mean_dims=[0], reduce_sum_dims=[1])
            return self

    class NICEFlow(nn.Module):
        def __init__(self):
            super().__init__()
            masks = inv.get_coupling_mask(Z_DIM, 1, 3)
            self.flow = inv.RevSequential([inv.MaskCoupling(Z_DIM, H, 2, masks[i].to(device)) for i in range(3)] + [inv.Scaling(Z_DIM)])

        def forward(self, z, **kwargs):
            out, log_det_J = self.flow.forward(z[0], **kwargs)
            return {"z": out}, log_det_J
    return ELBO(Generator(), Variational(), transform=NICEFlow(), transform_var=['z'])
