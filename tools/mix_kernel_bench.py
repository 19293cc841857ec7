#!/usr/bin/env python
"""The mixture-of-Gaussians density (include/zs_mix.h: NormalMixture.log_prob and its gradients on the matrix-core kernels)
against two torch compositions of the same expression on the same GPU and the same operands.

    python tools/mix_kernel_bench.py [--steps 3] [--warmup 1] [--repeats 3] [--rows 256 12800 102400]

Shapes: rows in {256, 12 800, 102 400}, D in {8, 40, 64}, C in {16, 64, 500}, float32.  Three measurements per shape, each the
forward plus what it names:

    forward      log_prob under no_grad
    grad_x       log_prob, then backward with only x requiring a gradient (a frozen prior)
    grad_all     log_prob, then backward with x, logits, mean and logstd requiring gradients (a learned prior)

    fused        the kernels of libzs_mix.so (prologue, main and finish launches)
    matmul       zhusuan.distributions._mix_functions.torch_log_prob: the expanded square as one [rows, 2 D] x [2 D, C] product
    broadcast    what users write today: ((x[:, None, :] - mean) / std) ** 2 summed over D, torch.logsumexp; not run where one
                 [rows, C, D] temporary exceeds 2^31 elements (reported as null)

After `warmup` steps of every variant the variants alternate in `repeats` rounds of one block of `steps` steps each, so that drift
of the box hits all alike.  A block is timed with device events around the enqueued work; the figure is milliseconds per step at
the median over the blocks, with the ratios torch / fused at the medians.  `peak_bytes` is what one step allocates above the
operands (torch.cuda.max_memory_allocated around it).  Nothing here is asserted by a test; bench.py is the project's yardstick and
is not involved.  Prints one JSON line per shape and measurement."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zhusuan-pytorch_amd"))

import torch  # noqa: E402

DIMS, COMPONENTS = [8, 40, 64], [16, 64, 500]


def broadcast_log_prob(logits, mean, logstd, x):
    z = (x[:, None, :] - mean) / torch.exp(logstd)
    comp = (-0.5 * z * z - logstd - 0.5 * math.log(2.0 * math.pi)).sum(-1) + torch.log_softmax(logits, 0)
    return torch.logsumexp(comp, -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rows", type=int, nargs="+", default=[256, 12800, 102400])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mix_kernel_bench needs a HIP device: there is nothing to time without one")
    from zhusuan.distributions import NormalMixture
    from zhusuan.distributions import _mix_functions as F
    dev = torch.device("cuda:0")
    for R in args.rows:
        for D in DIMS:
            for C in COMPONENTS:
                gen = torch.Generator(device=dev).manual_seed(R + D + C)
                params = [torch.randn(C, generator=gen, device=dev), 2.0 * torch.randn(C, D, generator=gen, device=dev),
                          -1.0 + 0.5 * torch.randn(C, D, generator=gen, device=dev)]
                x = torch.randn(R, D, generator=gen, device=dev)
                for what in ("forward", "grad_x", "grad_all"):
                    x.requires_grad_(what != "forward")
                    for p in params:
                        p.requires_grad_(what == "grad_all")

                    def step(lp_of):
                        if what == "forward":
                            with torch.no_grad():
                                return lp_of()
                        x.grad = None
                        for p in params:
                            p.grad = None
                        lp = lp_of()
                        lp.sum().backward()
                        return lp

                    variants = [("fused", lambda: step(lambda: NormalMixture(params[0], params[1], logstd=params[2]).log_prob(x))),
                                ("matmul", lambda: step(lambda: F.torch_log_prob(*params, x)))]
                    if R * C * D < 2 ** 31:
                        variants.append(("broadcast", lambda: step(lambda: broadcast_log_prob(*params, x))))
                    last, peak = {}, {}
                    for n, run in variants:
                        for _ in range(args.warmup):
                            last[n] = run().detach()
                        torch.cuda.synchronize()
                        x.grad = None
                        base = torch.cuda.memory_allocated()
                        torch.cuda.reset_peak_memory_stats()
                        run()
                        torch.cuda.synchronize()
                        peak[n] = torch.cuda.max_memory_allocated() - base
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
                    out = dict(tool="mix_kernel_bench", what=what, rows=R, D=D, C=C, dtype="float32", steps=args.steps,
                               warmup=args.warmup, repeats=args.repeats, device=torch.cuda.get_device_name(0), unit="ms_per_step",
                               scores_bytes=4 * R * C,
                               max_abs_difference_to_matmul=float("%.3g" % float((last["fused"] - last["matmul"]).abs().max())))
                    for n in ("fused", "matmul", "broadcast"):
                        b = blocks.get(n)
                        out[n] = None if b is None else {"median": round(statistics.median(b), 3), "min": round(min(b), 3),
                                                         "max": round(max(b), 3), "peak_bytes": peak[n]}
                        if b is not None and n != "fused":
                            out[n + "_over_fused"] = round(out[n]["median"] / out["fused"]["median"], 2)
                    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
