"""Time and peak allocation of MultivariateNormalLowRank's log_prob forward + backward on the GPU: the fused kernels
(include/zs_lowrank.h) against the torch Woodbury composition (zhusuan.distributions._lowrank_functions.torch_log_prob) and against
torch.distributions.LowRankMultivariateNormal, float32, same device, same inputs.

    python tools/lowrank_kernel_bench.py > profiles/lowrank_kernel_bench.txt

Method: per shape and path, 20 warm-up iterations, then 7 batches of 50 iterations between two events; the median batch is
reported with the fastest and slowest next to it.  An iteration is log_prob of x [K, R, D] and the gradients of its sum for
mean, cov_factor, cov_diag and x.  Peak allocation is torch.cuda.max_memory_allocated over one iteration minus what was allocated
before it (the kernels' workspaces are torch tensors and are counted)."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zhusuan-pytorch_amd"))

from zhusuan.distributions import MultivariateNormalLowRank          # noqa: E402
from zhusuan.distributions._lowrank_functions import torch_log_prob          # noqa: E402

SHAPES = [(1, D, r, K) for D in (1000, 10000) for r in (8, 64) for K in (10, 100)] + [(256, 256, 16, 50)]
WARMUP, BATCHES, ITERS = 20, 7, 50


def paths(mean, W, d):
    return {"kernels": lambda x: MultivariateNormalLowRank(mean, W, d).log_prob(x),
            "composition": lambda x: torch_log_prob(mean, W, d, x),
            "torch.distributions": lambda x: torch.distributions.LowRankMultivariateNormal(mean, W, d, validate_args=False).log_prob(x)}


def measure(fn, leaves):
    def step():
        torch.autograd.grad(fn(leaves[3]).sum(), leaves)
    for _ in range(WARMUP):
        step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    times = []
    for _ in range(BATCHES):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(ITERS):
            step()
        t1.record()
        torch.cuda.synchronize()
        times.append(1000.0 * t0.elapsed_time(t1) / ITERS)
    return statistics.median(times), min(times), max(times), peak


def main():
    dev = torch.device("cuda:0")
    print("device: %s; log_prob forward + backward, float32; us per iteration: median (min .. max) of %d batches of %d; peak KiB"
          % (torch.cuda.get_device_name(0), BATCHES, ITERS))
    print("%5s %6s %3s %4s  %-20s %10s %22s %10s" % ("R", "D", "r", "K", "path", "us", "(min .. max)", "peak KiB"))
    for R, D, r, K in SHAPES:
        g = torch.Generator().manual_seed(D + r + K)
        mean, W = torch.randn(R, D, generator=g), torch.randn(R, D, r, generator=g) / r ** 0.5
        d, x = 0.3 + torch.rand(R, D, generator=g), torch.randn(K, R, D, generator=g)
        leaves = [t.to(dev).requires_grad_(True) for t in (mean, W, d, x)]
        for name, fn in paths(*leaves[:3]).items():
            med, lo, hi, peak = measure(fn, leaves)
            print("%5d %6d %3d %4d  %-20s %10.1f %22s %10.1f" % (R, D, r, K, name, med, "(%.1f .. %.1f)" % (lo, hi), peak / 1024.0))


if __name__ == "__main__":
    main()
