"""Fixtures of the sampler tests: trajectories of the REFERENCE's SGLD / PSGLD / SGHMC on a small BNN (tests/mcmc_models.py).

    python tests/golden/mcmc/gen_mcmc_golden.py [--ref /path/to/reference] [--out DIR]

Only imports and calls the reference (its ``zhusuan.mcmc`` and ``zhusuan.framework``); nothing of it is stored but data.
In this process only, ``torch.normal`` is replaced by a wrapper that draws ``z = torch.normal(0., 1., size=shape)``, records
``z`` and returns ``mean + std * z``: every draw of a run -- the prior draws of ``resample=True`` (two per latent: the node's own
and the sampler's re-read of ``node.tensor``) and the samplers' noise -- becomes one list of standard normals in call order,
which ``zhusuan.inject_epsilon`` can hand to this package.  The run is made in float32, then the SAME draws are replayed
through the reference in float64.  Per case the file holds: x, y, the torch seed, the draws, the float32 latents after the
resample call and after each of the updates, and gap[t] = max |q32_t - q64_t| over all latents: the reference's own rounding
distance, which the tests' tolerance is built on."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import mcmc_models as M  # noqa: E402

SEEDS = {"sgld": 11, "psgld": 12, "sghmc_first_order": 13, "sghmc_second_order": 14}
_orig_normal = torch.normal


class Draws(object):
    """Recording (replay is None) or replaying wrapper of torch.normal."""

    def __init__(self, dtype, replay=None):
        self.dtype, self.replay, self.made = dtype, (list(replay) if replay is not None else None), []

    def __call__(self, mean, std=None, *, size=None, **kw):
        if size is not None:
            shape = tuple(size)
        else:
            shape = tuple(torch.broadcast_shapes(*[tuple(t.shape) for t in (mean, std) if isinstance(t, torch.Tensor)]))
        if self.replay is None:
            z = _orig_normal(0., 1., size=shape)
        else:
            z = torch.as_tensor(self.replay.pop(0))
            assert tuple(z.shape) == shape, (tuple(z.shape), shape)
        self.made.append(z.numpy().copy())
        return mean + std * z.to(self.dtype)


def run(ref_mcmc, ref_bn, case, dtype, x, y, seed, replay=None):
    cls, kw, layers = M.CASES[case]
    draws = Draws(dtype, replay)
    torch.normal = draws
    try:
        torch.manual_seed(seed)
        net = M.make_net(ref_bn, layers, dtype=dtype)
        sampler = getattr(ref_mcmc, cls)(M.LR, **kw)
        obs = {'x': torch.as_tensor(x, dtype=dtype), 'y': torch.as_tensor(y, dtype=dtype)}
        traj = []
        out = sampler.sample(net, obs, resample=True)
        names = list(out.keys())
        traj.append([out[k].detach().numpy().copy() for k in names])
        for _ in range(M.N_UPDATES):
            out = sampler.sample(net, obs)
            traj.append([out[k].detach().numpy().copy() for k in names])
    finally:
        torch.normal = _orig_normal
    return names, traj, draws.made


def generate(out_dir, ref_root):
    sys.path.insert(0, ref_root)
    for m in [k for k in sys.modules if k == "zhusuan" or k.startswith("zhusuan.")]:
        del sys.modules[m]
    import zhusuan.mcmc as ref_mcmc
    from zhusuan.framework.bn import BayesianNet as ref_bn
    assert ref_mcmc.__file__.startswith(ref_root), ref_mcmc.__file__
    os.makedirs(out_dir, exist_ok=True)
    for case, (cls, kw, layers) in M.CASES.items():
        seed = SEEDS[case]
        x, y = M.make_data(seed, layers[0])
        names, t32, draws = run(ref_mcmc, ref_bn, case, torch.float32, x, y, seed)
        names64, t64, draws64 = run(ref_mcmc, ref_bn, case, torch.float64, x, y, seed, replay=draws)
        assert names == names64 and len(draws) == len(draws64)
        gap = np.array([max(float(np.abs(a.astype(np.float64) - b).max()) for a, b in zip(s32, s64))
                        for s32, s64 in zip(t32, t64)])
        arrays = dict(x=x, y=y, seed=np.int64(seed), n_draws=np.int64(len(draws)), names=np.array(names), gap=gap)
        for i, z in enumerate(draws):
            arrays["draw_%02d" % i] = z
        for t, step in enumerate(t32):
            for k, q in zip(names, step):
                arrays["q_%d_%s" % (t, k)] = q
        np.savez(os.path.join(out_dir, "g_mcmc_%s.npz" % case), **arrays)
        print("%-20s %2d draws  max|q| %.3f  gap %s" % (case, len(draws), max(float(np.abs(q).max()) for q in t32[-1]),
                                                        " ".join("%.1e" % g for g in gap)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    generate(a.out, a.ref)
