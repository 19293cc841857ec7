#!/usr/bin/env python
"""MatrixVariateNormalCholesky (include/zs_matvar.h: the draw with its density, the density of a given value, and both backwards,
on the matrix-core kernels) against the torch composition of the same expressions on the same GPU and the same operands.

    python tools/matvar_kernel_bench.py [--steps 20] [--warmup 5] [--repeats 5]

Shapes: (n, p) in {(16, 16), (51, 50), (128, 128)}, R in {1, 64} rows, K in {1, 10, 50} particles, float32.  Four measurements:

    M1       sample(K) and log_prob of the draw under no_grad
    M1+bwd   the same with gradients for mean, u_tril and v_tril, from a loss that uses the draw and its density
    M2       log_prob of a given [K, R, n, p] value under no_grad
    M2+bwd   the same with gradients for the three parameters and the value

    fused    the kernels of libzs_matvar.so (one launch forward; main and finish launches backward)
    torch    tril, matmul, solve_triangular, diagonal, log, sum and autograd's backward of those
             (zhusuan.distributions._matvar_functions.torch_sample / torch_log_prob) with torch.randn for the noise

After `warmup` steps of every variant the variants alternate in `repeats` rounds of one block of `steps` steps each, so that
drift of the box hits both alike.  A block is timed with device events around the enqueued work; the figure is milliseconds per
step, min / median / max over the blocks, with the torch / fused ratio at the medians.  Nothing here is asserted by a test;
bench.py is the project's yardstick and is not involved.  Prints one JSON line per shape and measurement."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zhusuan-pytorch_amd"))

import torch  # noqa: E402

EVENTS = [(16, 16), (51, 50), (128, 128)]
ROWS = [1, 64]
PARTICLES = [1, 10, 50]


def factor(shape, gen, dev):
    d = shape[-1]
    raw = torch.randn(shape, generator=gen, device=dev)
    return 0.5 / d ** 0.5 * torch.tril(raw, -1) + torch.diag_embed(0.5 + 1.5 * torch.rand(shape[:-1], generator=gen, device=dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("matvar_kernel_bench needs a HIP device: there is nothing to time without one")
    from zhusuan.distributions import MatrixVariateNormalCholesky
    from zhusuan.distributions import _matvar_functions as F
    dev = torch.device("cuda:0")
    for n, p in EVENTS:
        for R in ROWS:
            for K in PARTICLES:
                gen = torch.Generator(device=dev).manual_seed(1000 * n + 10 * R + K)
                mean = torch.randn(R, n, p, generator=gen, device=dev)
                U, V = factor((R, n, n), gen, dev), factor((R, p, p), gen, dev)
                x = mean + 2.0 * torch.randn(K, R, n, p, generator=gen, device=dev)
                for what in ("M1", "M1+bwd", "M2", "M2+bwd"):
                    grad = what.endswith("bwd")
                    leaves = [t.clone().requires_grad_(grad) for t in (mean, U, V, x)]

                    def fused():
                        d = MatrixVariateNormalCholesky(*leaves[:3])
                        if what.startswith("M1"):
                            z = d.sample(K)
                            return z, d.log_prob(z)
                        return None, d.log_prob(leaves[3])

                    def composed():
                        if what.startswith("M1"):
                            return F.torch_sample(leaves[0], leaves[1], leaves[2], torch.randn(K, R, n, p, device=dev))
                        return None, F.torch_log_prob(*leaves)

                    def step(forward):
                        with torch.set_grad_enabled(grad):
                            z, lp = forward()
                            if grad:
                                for t in leaves:
                                    t.grad = None
                                (lp.sum() if z is None else lp.sum() + z.sum()).backward()
                        return lp

                    variants = [("fused", lambda: step(fused)), ("torch", lambda: step(composed))]
                    for _, run in variants:
                        for _ in range(args.warmup):
                            run()
                    torch.cuda.synchronize()
                    blocks = dict((name, []) for name, _ in variants)
                    for _ in range(args.repeats):
                        for name, run in variants:
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            for _ in range(args.steps):
                                run()
                            e1.record()
                            torch.cuda.synchronize()
                            blocks[name].append(e0.elapsed_time(e1) / args.steps)
                    out = dict(tool="matvar_kernel_bench", what=what, n=n, p=p, R=R, K=K, dtype="float32", steps=args.steps,
                               warmup=args.warmup, repeats=args.repeats, device=torch.cuda.get_device_name(0), unit="ms_per_step")
                    for name, _ in variants:
                        b = blocks[name]
                        out[name] = {"min": round(min(b), 4), "median": round(statistics.median(b), 4), "max": round(max(b), 4)}
                    out["torch_over_fused"] = round(out["torch"]["median"] / out["fused"]["median"], 2)
                    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
