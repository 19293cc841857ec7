#!/usr/bin/env python
"""The inclusive-KL objective (Q1 of include/zs_klpq.h), forward + backward, against the same objective written with torch
operations on the same GPU and the same inputs.

    python tools/klpq_kernel_bench.py [--steps 50] [--warmup 10] [--repeats 7]

Shapes (K, B, Tp, Tq): (50, 256, 3, 2) -- the size DESIGN.md section 5 trains at --, (8, 1024, 3, 2), and (50, 4096, 3, 2), whose
batch is beyond the one-workgroup mean: there the fused step is the launch, torch's mean, its backward and the backward launch.

A step takes Tp + Tq log-probability matrices [K, B] that require gradients, forms the batch-mean cost and backpropagates it
into every term (``model_grad=True``: the generator's terms receive a gradient too):

    fused    InclusiveKLObjective.importance: one launch of libzs_klpq.so forward, one backward
    torch    zhusuan.variational.inclusive_kl.torch_composition, the composition a layout outside the kernel runs: the additions
             of the two log-joints, subtract, max, exp, sum, divide, multiply, where, sum, mean, and autograd's backward of them

After `warmup` steps of every variant the variants alternate in `repeats` rounds of one block of `steps` steps each, so that
drift of the box hits both alike.  A block is timed with device events around the enqueued work (kernels and the gaps between
them), the figure is microseconds per step, and min / median / max over the blocks are reported with the torch / fused ratio at
the medians.  These are times of whole launch-bound Python steps; the kernels' own durations are not measured here.  Nothing
here is asserted by a test; bench.py is the project's yardstick and is not involved.  Prints one JSON line per case."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zhusuan-pytorch_amd"))

import torch  # noqa: E402

SHAPES = [(50, 256, 3, 2), (8, 1024, 3, 2), (50, 4096, 3, 2)]


def cases(K, B, Tp, Tq, dev):
    from zhusuan.variational import InclusiveKLObjective
    from zhusuan.variational.inclusive_kl import torch_composition
    gen = torch.Generator().manual_seed(K + B)
    tp = [(2.0 * torch.randn(K, B, generator=gen) - 30.0).to(dev).requires_grad_(True) for _ in range(Tp)]
    tq = [(2.0 * torch.randn(K, B, generator=gen) - 10.0).to(dev).requires_grad_(True) for _ in range(Tq)]
    obj = InclusiveKLObjective(None, None, axis=0, model_grad=True)

    def fused():
        obj.importance(tp, tq).backward()

    def eager():
        torch_composition(tp, tq, 0, True)[0].mean().backward()

    return tp + tq, fused, eager


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("klpq_kernel_bench needs a HIP device: there is nothing to time without one")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    for K, B, Tp, Tq in SHAPES:
        leaves, fused, eager = cases(K, B, Tp, Tq, dev)

        def clear():
            for t in leaves:
                t.grad = None
        variants = [("fused", fused), ("torch", eager)]
        grads = {}
        for n, step in variants:
            for _ in range(args.warmup):
                clear()
                step()
            grads[n] = [t.grad.clone() for t in leaves]
        torch.cuda.synchronize()
        # the two variants compute the same thing: the largest gradient difference relative to the largest gradient
        diff = max(float((a - b).abs().max()) for a, b in zip(grads["fused"], grads["torch"]))
        scale = max(float(b.abs().max()) for b in grads["torch"])
        blocks = dict((n, []) for n, _ in variants)
        for _ in range(args.repeats):
            for n, step in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    clear()
                    step()
                e1.record()
                torch.cuda.synchronize()
                blocks[n].append(e0.elapsed_time(e1) * 1e3 / args.steps)
        out = dict(tool="klpq_kernel_bench", K=K, B=B, Tp=Tp, Tq=Tq, steps=args.steps, warmup=args.warmup, repeats=args.repeats,
                   device=torch.cuda.get_device_name(0), unit="us_per_forward_plus_backward",
                   max_gradient_difference_relative=float("%.3g" % (diff / scale)))
        for n, _ in variants:
            b = blocks[n]
            out[n] = {"min": round(min(b), 1), "median": round(statistics.median(b), 1), "max": round(max(b), 1)}
        out["torch_over_fused"] = round(out["torch"]["median"] / out["fused"]["median"], 2)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
