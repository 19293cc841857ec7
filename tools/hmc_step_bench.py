#!/usr/bin/env python
"""One HMC iteration (L = 10), fused kernels against the same iteration written with torch operations on the device.

    python tools/hmc_step_bench.py [--steps 30] [--warmup 5] [--repeats 5] [--leapfrogs 10] [--chains 1000]

Workloads:

    bnn      examples/bnn_sgmcmc.py's net, layer sizes [13, 50, 1], 20 particles, batch 114: two latents, 14 000 + 1 020
             elements, a scalar log joint (one chain)
    big      a single latent of 10^6 elements, `chains` chains of 10^6 / chains elements, a Gaussian log joint in torch ops

Variants, all around the SAME L + 1 evaluations of the log joint and its gradient:

    fused    zhusuan.mcmc.HMC: L + 3 launches of libzs_hmc.so per iteration (BEGIN, L - 1 STEP, END, decide, select)
    eager    the restatement of tests/hmc_host.py moved to the device: torch.randn, per latent the leapfrog as mul / add, the
             kinetic energies as square-and-sum, exp / log / where for the decision.  There is no HMC before this library, so
             this is the only comparison there is.
    grads    the L + 1 evaluations alone: what both of the above contain

After `warmup` iterations of every variant the variants alternate in `repeats` rounds of one block of `steps` iterations each,
so that drift of the box hits all of them alike.  A block is timed on the host around a device synchronisation, the figure is
microseconds per iteration, and min / median / max over the blocks are reported.  `outside_log_joint` is 1 - grads / variant
at the medians.  Nothing here is asserted by a test; bench.py is the project's yardstick and is not involved.
Prints one JSON line per workload."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zhusuan-pytorch_amd"))

import torch  # noqa: E402


def eager_iteration(logp_and_grad, q0, eps, L):
    """tests/hmc_host.py's reference iteration with torch ops on the device; returns the selected state."""
    logp0, g = logp_and_grad(q0)
    C = max(logp0.numel(), 1)
    z = [torch.randn_like(t) for t in q0]
    u = torch.rand(C, device=q0[0].device, dtype=logp0.dtype)
    k0 = 0.5 * sum((t * t).reshape(C, -1).sum(dim=1) for t in z)
    p = [t + (0.5 * eps) * gi for t, gi in zip(z, g)]
    q = [a + eps * b for a, b in zip(q0, p)]
    for _ in range(L - 1):
        _, g = logp_and_grad(q)
        p = [a + eps * gi for a, gi in zip(p, g)]
        q = [a + eps * b for a, b in zip(q, p)]
    logp1, g = logp_and_grad(q)
    pl = [a + (0.5 * eps) * gi for a, gi in zip(p, g)]
    k1 = 0.5 * sum((t * t).reshape(C, -1).sum(dim=1) for t in pl)
    dh = (logp1.reshape(-1) - logp0.reshape(-1)) - (k1 - k0)
    acc = torch.isfinite(dh) & (torch.log(u) < dh)
    return [torch.where(acc.view([C] + [1] * (a.reshape(C, -1).dim() - 1)), b.reshape(C, -1), a.reshape(C, -1)).view(a.shape)
            for a, b in zip(q0, q)]


def eager_ops(n_latents, L):
    """torch operations of eager_iteration outside the log joint, each at least one kernel launch."""
    per_latent = 1 + 2 + 4 + 4 * (L - 1) + 2 + 2 + 1          # randn, K0, begin, steps, end, K1, where
    return n_latents * per_latent + 8                          # rand, dH (3), isfinite, log, <, &


def measure(name, make_net_obs_latent, args, extra):
    from zhusuan import _hmc_hip
    from zhusuan.mcmc import HMC
    net, obs, names, start = make_net_obs_latent()
    L, eps = args.leapfrogs, args.step_size

    launches = [0]
    inner = (_hmc_hip.move, _hmc_hip.decide, _hmc_hip.select)

    def wrap(fn):
        def f(*a, **k):
            launches[0] += 1
            return fn(*a, **k)
        return f
    _hmc_hip.move, _hmc_hip.decide, _hmc_hip.select = [wrap(f) for f in inner]

    def logp_and_grad(qs):
        return HMC._log_joint_and_grad(net, obs, names, qs)

    def fused():
        h = HMC(step_size=eps, n_leapfrogs=L)
        state = {"latent": dict(zip(names, [t.clone() for t in start]))}

        def step():
            state["latent"], _ = h.sample(net, obs, state["latent"])
        return step

    def eager():
        state = {"q": [t.clone() for t in start]}

        def step():
            state["q"] = eager_iteration(logp_and_grad, state["q"], eps, L)
        return step

    def grads():
        q = [t.clone() for t in start]

        def step():
            for _ in range(L + 1):
                logp_and_grad(q)
        return step

    steps_of = [("fused", fused()), ("eager", eager()), ("grads", grads())]
    for _, step in steps_of:
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()
    blocks = dict((n, []) for n, _ in steps_of)
    counted = 0
    for _ in range(args.repeats):
        for n, step in steps_of:
            launches[0] = 0
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            blocks[n].append((time.perf_counter() - t0) * 1e6 / args.steps)
            if n == "fused":
                counted += launches[0]
    _hmc_hip.move, _hmc_hip.decide, _hmc_hip.select = inner
    out = dict(tool="hmc_step_bench", workload=name, leapfrogs=L, steps=args.steps, warmup=args.warmup, repeats=args.repeats,
               device=torch.cuda.get_device_name(0), unit="us_per_iteration", **extra)
    for n, _ in steps_of:
        b = blocks[n]
        out[n] = {"min": round(min(b), 1), "median": round(statistics.median(b), 1), "max": round(max(b), 1)}
    g = out["grads"]["median"]
    out["library_launches_per_iteration"] = counted / float(args.repeats * args.steps)
    out["eager_torch_ops_per_iteration"] = eager_ops(len(names), L)
    out["outside_log_joint"] = {"fused": round(1 - g / out["fused"]["median"], 3), "eager": round(1 - g / out["eager"]["median"], 3)}
    out["speedup_eager_over_fused"] = round(out["eager"]["median"] / out["fused"]["median"], 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--leapfrogs", type=int, default=10)
    ap.add_argument("--step_size", type=float, default=1e-3)
    ap.add_argument("--chains", type=int, default=1000)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)

    def bnn():
        from examples import bnn_sgmcmc
        from zhusuan.mcmc import SGLD
        g = torch.Generator().manual_seed(1)
        obs = {"x": torch.randn(114, 13, generator=g).to(dev), "y": torch.randn(114, generator=g).to(dev)}
        net = bnn_sgmcmc.Net([13, 50, 1], 20, multiplier=456).to(dev)
        first = SGLD(1e-3).sample(net, obs, resample=True)
        return net, obs, ["w0", "w1"], [first[k].detach().clone() for k in ("w0", "w1")]

    def big():
        from zhusuan.framework.bn import BayesianNet
        C = args.chains
        row = 1000000 // C

        class Net(BayesianNet):
            def forward(self, observed):
                self.observe(observed)
                return self

            def _log_joint(self):
                x = self.observed["x"]
                return (-0.5 * x * x).sum(-1)
        return Net().to(dev), {}, ["x"], [torch.randn(C, row, device=dev)]

    measure("bnn", bnn, args, dict(latents=[14000, 1020], chains=1))
    measure("big", big, args, dict(latents=[1000000 // args.chains * args.chains], chains=args.chains))


if __name__ == "__main__":
    main()
