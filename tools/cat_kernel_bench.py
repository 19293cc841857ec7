#!/usr/bin/env python
"""The categorical draw (C1) and the relaxed draw (C3), forward + backward, against the same node written with torch operations
on the same GPU.

    python tools/cat_kernel_bench.py [--steps 50] [--warmup 10] [--repeats 7]

Shapes (K, R, N): (50, 256 * 20, 10), (50, 256, 1000), (1, 4096, 10).

Variants, each one "draw a [K, R, N] node from logits [R, N], take its log-probability, backpropagate sum(g * lp) (and, for the
relaxed node, sum(gz * z)) into logits":

    fused    zhusuan.distributions.OnehotCategorical / ExpConcrete: one launch of libzs_cat.so forward, one backward
    torch    OnehotCategorical: torch.rand, two logs, add, argmax, one_hot, log_softmax, multiply, sum, autograd's backward of it;
             ExpConcrete: torch.distributions.relaxed_categorical.ExpRelaxedCategorical.rsample + log_prob and autograd

After `warmup` steps of every variant the variants alternate in `repeats` rounds of one block of `steps` steps each, so that
drift of the box hits both alike.  A block is timed with device events around the enqueued work (kernels and the gaps between
them; the host is ahead of the device for all but the smallest shape, where the figure is the launch-bound step time), the
figure is microseconds per step, and min / median / max over the blocks are reported with the torch / fused ratio at the medians.
Nothing here is asserted by a test; bench.py is the project's yardstick and is not involved.  Prints one JSON line per case."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zhusuan-pytorch_amd"))

import torch  # noqa: E402
from torch.distributions import relaxed_categorical as trc  # noqa: E402

SHAPES = [(50, 256 * 20, 10), (50, 256, 1000), (1, 4096, 10)]
TAU = 0.67


def cases(K, R, N, dev):
    from zhusuan.distributions import OnehotCategorical, ExpConcrete
    gen = torch.Generator().manual_seed(K + R + N)
    logits = torch.randn(R, N, generator=gen).to(dev).requires_grad_(True)
    g = torch.randn(K, R, generator=gen).to(dev)
    gz = torch.randn(K, R, N, generator=gen).to(dev)
    tau = torch.tensor(TAU, device=dev)

    def c1_fused():
        d = OnehotCategorical(logits)
        z = d.sample(K)
        (g * d.log_prob(z).reshape(K, R)).sum().backward()

    def c1_torch():
        u = torch.rand(K, R, N, device=dev)
        idx = (logits.detach() - torch.log(-torch.log(u))).argmax(-1)
        z = torch.nn.functional.one_hot(idx, N).to(logits.dtype)
        lp = (z * torch.log_softmax(logits, -1)).sum(-1)
        (g * lp).sum().backward()

    def c3_fused():
        d = ExpConcrete(TAU, logits)
        y = d.sample(K).reshape(K, R, N)
        ((g * d.log_prob(None).reshape(K, R)).sum() + (gz * y).sum()).backward()

    def c3_torch():
        d = trc.ExpRelaxedCategorical(tau, logits=logits, validate_args=False)
        y = d.rsample((K,))
        ((g * d.log_prob(y)).sum() + (gz * y).sum()).backward()

    return logits, [("C1", c1_fused, c1_torch), ("C3", c3_fused, c3_torch)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cat_kernel_bench needs a HIP device: there is nothing to time without one")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    for K, R, N in SHAPES:
        logits, pairs = cases(K, R, N, dev)
        for name, fused, eager in pairs:
            variants = [("fused", fused), ("torch", eager)]
            for _, step in variants:
                for _ in range(args.warmup):
                    logits.grad = None
                    step()
            torch.cuda.synchronize()
            blocks = dict((n, []) for n, _ in variants)
            for _ in range(args.repeats):
                for n, step in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.steps):
                        logits.grad = None
                        step()
                    e1.record()
                    torch.cuda.synchronize()
                    blocks[n].append(e0.elapsed_time(e1) * 1e3 / args.steps)
            out = dict(tool="cat_kernel_bench", kernel=name, K=K, R=R, N=N, steps=args.steps, warmup=args.warmup, repeats=args.repeats,
                       device=torch.cuda.get_device_name(0), unit="us_per_forward_plus_backward")
            for n, _ in variants:
                b = blocks[n]
                out[n] = {"min": round(min(b), 1), "median": round(statistics.median(b), 1), "max": round(max(b), 1)}
            out["torch_over_fused"] = round(out["torch"]["median"] / out["fused"]["median"], 2)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
