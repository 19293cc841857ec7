"""Time and peak allocation of GPConditional's moments on the GPU, forward and forward + backward: the fused kernels
(include/zs_gp.h) against the torch composition of the same formula (zhusuan.distributions._gp_functions.torch_moments), float32,
same device, same inputs.

    python tools/gp_kernel_bench.py > profiles/gp_kernel_bench.txt

Method: per shape and path, 5 warm-up iterations, then 5 batches of 10 iterations between two events; the median batch is reported
with the fastest and slowest next to it.  An iteration is mean [K, N] and var [N] and, with the backward, the gradients of
sum(mean) + sum(var) for x, the inducing inputs, the lengthscales, the amplitude, the factor and f_inducing.  Peak allocation is
torch.cuda.max_memory_allocated over one forward + backward minus what was allocated before it (the kernels' workspaces are torch
tensors and are counted); N M elements of float32 are printed next to it."""
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zhusuan-pytorch_amd"))

from zhusuan.distributions import GPConditional          # noqa: E402
from zhusuan.distributions._gp_functions import torch_moments          # noqa: E402

SHAPES = [(N, M, d, K) for N in (256, 12800, 102400) for M in (16, 64, 128) for d in (1, 8, 64) for K in (1, 50)]
WARMUP, BATCHES, ITERS = 5, 5, 10


def kernels(x, Z, l, a, L, fz):
    dist = GPConditional(x, Z, fz, L, l, a)
    return dist.mean, dist.var


def composition(x, Z, l, a, L, fz):
    return torch_moments(x, Z, l, a.reshape(1), L, fz)


def timed(step):
    for _ in range(WARMUP):
        step()
    torch.cuda.synchronize()
    times = []
    for _ in range(BATCHES):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(ITERS):
            step()
        t1.record()
        torch.cuda.synchronize()
        times.append(1000.0 * t0.elapsed_time(t1) / ITERS)
    return statistics.median(times), min(times), max(times)


def measure(fn, leaves):
    def forward():
        with torch.no_grad():
            fn(*leaves)

    def both():
        mean, var = fn(*leaves)
        torch.autograd.grad(mean.sum() + var.sum(), leaves)
    fwd, fb = timed(forward), timed(both)
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    both()
    torch.cuda.synchronize()
    return fwd, fb, torch.cuda.max_memory_allocated() - base


def main():
    dev = torch.device("cuda:0")
    print("device: %s; GPConditional moments, float32; us per iteration: median (min .. max) of %d batches of %d; peak KiB of one "
          "forward + backward" % (torch.cuda.get_device_name(0), BATCHES, ITERS))
    print("%7s %4s %3s %3s  %-12s %10s %20s %10s %20s %10s %10s" % ("N", "M", "d", "K", "path", "fwd us", "(min .. max)", "fwd+bwd us",
                                                                   "(min .. max)", "peak KiB", "N M KiB"))
    for N, M, d, K in SHAPES:
        g = torch.Generator().manual_seed(N + M + d + K)
        x, Z = 4.0 * torch.rand(N, d, generator=g), 4.0 * torch.rand(M, d, generator=g)
        l, a, fz = torch.full((d,), float(d) ** 0.5), torch.tensor(1.3), torch.randn(K, M, generator=g)
        L = GPConditional.gram_tril(Z, l, a, jitter=0.1)
        leaves = [t.to(dev).requires_grad_(True) for t in (x, Z, l, a, L, fz)]
        for name, fn in (("kernels", kernels), ("composition", composition)):
            fwd, fb, peak = measure(fn, leaves)
            print("%7d %4d %3d %3d  %-12s %10.1f %20s %10.1f %20s %10.1f %10.1f"
                  % (N, M, d, K, name, fwd[0], "(%.1f .. %.1f)" % fwd[1:], fb[0], "(%.1f .. %.1f)" % fb[1:], peak / 1024.0, N * M * 4 / 1024.0))


if __name__ == "__main__":
    main()
