#!/usr/bin/env python
"""The admixture likelihood (include/zs_topic.h: AdmixtureMultinomial.log_prob and its two gradients on the matrix-core kernels)
against the torch composition of the same expression on the same GPU and the same operands.

    python tools/topic_kernel_bench.py [--steps 5] [--warmup 2] [--repeats 5]

Shapes: R in {100, 1000} rows (chains x documents), K = 50 topics, V = 12 419 words (the tutorial's vocabulary), float32, counts
~ Poisson(0.02) shared by all rows (Dx = R / 4).  Three measurements per shape, each the forward plus what it names:

    forward      log_prob under no_grad
    grad_doc     log_prob, then backward with only the document logits requiring a gradient (the HMC E-step)
    grad_topic   log_prob, then backward with only the topic logits requiring a gradient (the M-step)

    fused    the kernels of libzs_topic.so (prologue, main and finish launches)
    torch    softmax, matmul, log, multiply, row sum and autograd's backward of those (zhusuan.distributions._topic_functions)

After `warmup` steps of every variant the variants alternate in `repeats` rounds of one block of `steps` steps each, so that
drift of the box hits both alike.  A block is timed with device events around the enqueued work; the figure is milliseconds per
step, min / median / max over the blocks, with the torch / fused ratio at the medians.  `model` holds what follows from the shapes
alone: the FLOPs of the products (2 R K V forward, as many again for each second product) and the bytes either path must move at
least (the fused path: H, B, X and the thin outputs; the torch path: the same plus the [R, V] matrix written and read once per
pass: product, logarithm, weighted sum, and twice more in a backward).  Nothing here is asserted by a test; bench.py is the
project's yardstick and is not involved.  Prints one JSON line per shape and measurement."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zhusuan-pytorch_amd"))

import torch  # noqa: E402

K, V = 50, 12419
ROWS = [100, 1000]


def model(R, what):
    """FLOPs and minimum bytes (float32) from the shapes alone."""
    operands = 4 * (R * K + K * V + (R // 4) * V)
    thin = {"forward": 4 * R, "grad_doc": 4 * (R + R * K), "grad_topic": 4 * (R + K * V)}[what]
    rv = 4 * R * V
    passes = {"forward": 5, "grad_doc": 9, "grad_topic": 9}[what]          # [R, V] written or read, torch path
    products = {"forward": 1, "grad_doc": 3, "grad_topic": 3}[what]          # the product again in the backward, and the second one
    return dict(flops=2 * R * K * V * products, fused_min_bytes=operands + thin, torch_min_bytes=operands + thin + passes * rv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topic_kernel_bench needs a HIP device: there is nothing to time without one")
    from zhusuan.distributions import AdmixtureMultinomial
    from zhusuan.distributions import _topic_functions as F
    dev = torch.device("cuda:0")
    for R in ROWS:
        gen = torch.Generator(device=dev).manual_seed(R)
        H0 = torch.randn(R, K, generator=gen, device=dev)
        B0 = 2.0 * torch.randn(K, V, generator=gen, device=dev)
        X = torch.poisson(torch.full((R // 4, V), 0.02, device=dev), generator=gen)
        for what in ("forward", "grad_doc", "grad_topic"):
            H = H0.clone().requires_grad_(what == "grad_doc")
            B = B0.clone().requires_grad_(what == "grad_topic")

            def step(lp_of):
                if what == "forward":
                    with torch.no_grad():
                        return lp_of()
                H.grad = B.grad = None
                lp = lp_of()
                lp.sum().backward()
                return lp

            variants = [("fused", lambda: step(lambda: AdmixtureMultinomial(H.view(4, R // 4, K), B).log_prob(X))),
                        ("torch", lambda: step(lambda: F.torch_log_prob(H.view(4, R // 4, K), B, X)))]
            last = {}
            for n, run in variants:
                for _ in range(args.warmup):
                    last[n] = run().detach().reshape(-1)
            torch.cuda.synchronize()
            blocks = dict((n, []) for n, _ in variants)
            for _ in range(args.repeats):
                for n, run in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.steps):
                        run()
                    e1.record()
                    torch.cuda.synchronize()
                    blocks[n].append(e0.elapsed_time(e1) / args.steps)
            out = dict(tool="topic_kernel_bench", what=what, R=R, K=K, V=V, Dx=R // 4, dtype="float32", steps=args.steps,
                       warmup=args.warmup, repeats=args.repeats, device=torch.cuda.get_device_name(0), unit="ms_per_step",
                       model=model(R, what),
                       max_relative_difference=float("%.3g" % float(((last["fused"] - last["torch"]) / last["torch"]).abs().max())))
            for n, _ in variants:
                b = blocks[n]
                out[n] = {"min": round(min(b), 3), "median": round(statistics.median(b), 3), "max": round(max(b), 3)}
            out["torch_over_fused"] = round(out["torch"]["median"] / out["fused"]["median"], 2)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
