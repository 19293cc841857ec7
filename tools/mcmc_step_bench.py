#!/usr/bin/env python
"""One BNN SGLD step at the reference example's size, fused update against the reference's update sequence.

    python tools/mcmc_step_bench.py [--steps 300] [--warmup 50] [--repeats 5] [--sampler sgld|psgld|sghmc]

Workload: examples/bnn_sgmcmc.py's net, layer sizes [13, 50, 1], 20 particles, batch 114 (the sizes of the reference's
examples/bayesian_neural_nets/bnn_sgmcmc.py:88-95): two latents, 14 000 + 1 020 elements.  Variants, all around the SAME
forward / log-joint / autograd.grad through the package's kernels:

    fused    zhusuan.mcmc's sampler: one launch of zs_mcmc_update over both latents (two for SGHMC)
    eager    the reference's update loop restated with torch ops on the device tensors (SGLD.py:49-54): per latent a host
             torch.normal copied to the device, the element-wise update, detach, requires_grad (SGLD only)
    grad     the gradient alone, no update: what both of the above contain

After `warmup` steps of every variant the variants alternate in `repeats` rounds of one block of `steps` steps each, so
that drift of the box hits all of them alike (the step is host-bound: timed one variant after the other, whichever came
first read 130-200 us slower).  A block is timed on the host around a device synchronisation, the figure is microseconds
per step, and min / median / max over the blocks are reported, so the spread is visible next to the difference.  Nothing here is asserted by a test; bench.py is the project's yardstick and is not involved.
Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zhusuan-pytorch_amd"))

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sampler", default="sgld", choices=["sgld", "psgld", "sghmc"])
    ap.add_argument("--particles", type=int, default=20)
    ap.add_argument("--batch", type=int, default=114)
    args = ap.parse_args()

    from zhusuan import _mcmc_hip
    from examples import bnn_sgmcmc
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(args.batch, 13, generator=g).to(dev)
    y = torch.randn(args.batch, generator=g).to(dev)
    obs = {"x": x, "y": y}
    lr = 1e-3
    net = bnn_sgmcmc.Net([13, 50, 1], args.particles, multiplier=456).to(dev)

    launches = [0]
    inner = _mcmc_hip.update

    def counted(*a, **k):
        launches[0] += 1
        return inner(*a, **k)
    _mcmc_hip.update = counted

    def fused():
        s = bnn_sgmcmc.make_sampler(args.sampler, lr)
        s.sample(net, obs, resample=True)
        return lambda: s.sample(net, obs)

    def grads_of(qs):
        net.forward({"w0": qs[0], "w1": qs[1], **obs})
        return torch.autograd.grad(net.log_joint(), qs)

    def start():
        s = bnn_sgmcmc.make_sampler("sgld", lr)
        first = s.sample(net, obs, resample=True)
        return [first[k].detach().requires_grad_(True) for k in ("w0", "w1")]

    def eager():
        qs = start()

        def step():
            gr = grads_of(qs)
            for i in range(len(qs)):
                eps = torch.normal(0., math.sqrt(lr), size=qs[i].shape).to(dev)
                q = qs[i] + 0.5 * lr * gr[i] + eps
                q = q.detach()
                q.requires_grad = True
                qs[i] = q
        return step

    def grad_only():
        qs = start()
        return lambda: grads_of(qs)

    variants = [("fused", fused), ("grad", grad_only)] + ([("eager", eager)] if args.sampler == "sgld" else [])
    out = {"tool": "mcmc_step_bench", "sampler": args.sampler, "layer_sizes": [13, 50, 1], "particles": args.particles,
           "batch": args.batch, "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "unit": "us_per_step"}
    steps_of = [(name, make()) for name, make in variants]
    for name, step in steps_of:
        for _ in range(args.warmup):
            step()
    torch.cuda.synchronize()
    blocks = dict((name, []) for name, _ in steps_of)
    counted_launches = 0
    for _ in range(args.repeats):          # the variants alternate block by block: drift of the box hits all of them alike
        for name, step in steps_of:
            launches[0] = 0
            t0 = time.perf_counter()
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
            blocks[name].append((time.perf_counter() - t0) * 1e6 / args.steps)
            if name == "fused":
                counted_launches += launches[0]
    for name, _ in steps_of:
        b = blocks[name]
        out[name] = {"min": round(min(b), 2), "median": round(statistics.median(b), 2), "max": round(max(b), 2)}
    out["update_launches_per_step"] = counted_launches / float(args.repeats * args.steps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
