#!/usr/bin/env python
"""The multivariate-normal draw (V1) and the density of a given value (V2), forward + backward, against the same node written
with torch operations on the same GPU.

    python tools/mvn_kernel_bench.py [--steps 50] [--warmup 10] [--repeats 7]

Shapes (K, R, D): (50, 256, 40), (50, 5120, 8), (1, 4096, 64).

Variants, each one a whole step:

    V1  draw a [K, R, D] node from mean [R, D] and cov_tril [R, D, D], take its log-density, backpropagate
        sum(g * lp) + sum(gz * z) into mean and cov_tril
    V2  take the log-density of a given [K, R, D] value, backpropagate sum(g * lp) into mean, cov_tril and the value

    fused    zhusuan.distributions.MultivariateNormalCholesky: one launch of libzs_mvn.so forward, one backward
    torch    the composition the wide rows run: torch.randn, tril, batched matmul, add, diagonal, log, sum, square, sum (V1);
             tril, subtract, torch.linalg.solve_triangular, diagonal, log, sum, square, sum (V2); autograd's backward of them

After `warmup` steps of every variant the variants alternate in `repeats` rounds of one block of `steps` steps each, so that
drift of the box hits both alike.  A block is timed with device events around the enqueued work (kernels and the gaps between
them), the figure is microseconds per step, and min / median / max over the blocks are reported with the torch / fused ratio at
the medians.  Nothing here is asserted by a test; bench.py is the project's yardstick and is not involved.  Prints one JSON line
per case."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zhusuan-pytorch_amd"))

import torch  # noqa: E402

SHAPES = [(50, 256, 40), (50, 5120, 8), (1, 4096, 64)]


def cases(K, R, D, dev):
    from zhusuan.distributions import MultivariateNormalCholesky
    gen = torch.Generator().manual_seed(K + R + D)
    mean = (3.0 * torch.randn(R, D, generator=gen)).to(dev).requires_grad_(True)
    L = torch.tril(torch.randn(R, D, D, generator=gen) * 0.5 / math.sqrt(D), -1) + torch.diag_embed(0.5 + 1.5 * torch.rand(R, D, generator=gen))
    tril = L.to(dev).requires_grad_(True)
    x = (mean.detach().cpu()[None] + 2.0 * torch.randn(K, R, D, generator=gen)).to(dev).requires_grad_(True)
    g = torch.randn(K, R, generator=gen).to(dev)
    gz = torch.randn(K, R, D, generator=gen).to(dev)
    c0 = -0.5 * D * math.log(2.0 * math.pi)

    def v1_fused():
        d = MultivariateNormalCholesky(mean, tril)
        z = d.sample(K).reshape(K, R, D)
        ((g * d.log_prob(None).reshape(K, R)).sum() + (gz * z).sum()).backward()

    def v1_torch():
        eps = torch.randn(K, R, D, device=dev)
        Lt = torch.tril(tril)
        z = mean + (Lt @ eps[..., None])[..., 0]
        lp = c0 - torch.log(torch.diagonal(Lt, dim1=-2, dim2=-1)).sum(-1) - 0.5 * (eps * eps).sum(-1)
        ((g * lp).sum() + (gz * z).sum()).backward()

    def v2_fused():
        (g * MultivariateNormalCholesky(mean, tril).log_prob(x).reshape(K, R)).sum().backward()

    def v2_torch():
        Lt = torch.tril(tril)
        y = torch.linalg.solve_triangular(Lt.expand(K, R, D, D), (x - mean)[..., None], upper=False)[..., 0]
        lp = c0 - torch.log(torch.diagonal(Lt, dim1=-2, dim2=-1)).sum(-1) - 0.5 * (y * y).sum(-1)
        (g * lp).sum().backward()

    return [mean, tril, x], [("V1", v1_fused, v1_torch), ("V2", v2_fused, v2_torch)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mvn_kernel_bench needs a HIP device: there is nothing to time without one")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    for K, R, D in SHAPES:
        leaves, pairs = cases(K, R, D, dev)

        def clear():
            for t in leaves:
                t.grad = None
        for name, fused, eager in pairs:
            variants = [("fused", fused), ("torch", eager)]
            for _, step in variants:
                for _ in range(args.warmup):
                    clear()
                    step()
            torch.cuda.synchronize()
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
            out = dict(tool="mvn_kernel_bench", kernel=name, K=K, R=R, D=D, steps=args.steps, warmup=args.warmup, repeats=args.repeats,
                       device=torch.cuda.get_device_name(0), unit="us_per_forward_plus_backward")
            for n, _ in variants:
                b = blocks[n]
                out[n] = {"min": round(min(b), 1), "median": round(statistics.median(b), 1), "max": round(max(b), 1)}
            out["torch_over_fused"] = round(out["torch"]["median"] / out["fused"]["median"], 2)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
