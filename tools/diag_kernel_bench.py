#!/usr/bin/env python
"""The chain diagnostics (zs_diag_summary of include/zs_diag.h: mean, var+, split R-hat, effective sample size in one launch)
against the same estimator written with torch operations on the same GPU and the same draws.

    python tools/diag_kernel_bench.py [--steps 3] [--warmup 1] [--repeats 5] [--shapes all]

Shapes (T, C, E): (1000, 4, 10^4), (1000, 4, 10^6) and (200, 20, 6.5 10^5) -- a small and a large BNN posterior of four long
chains, and many short chains.  The draws are float32 AR(1) series generated on the device, phi from -0.5 to 0.9 over the
elements, so the lag loop stops early for most elements and late for some.

    fused    zhusuan.diagnostics.summary: one launch of libzs_diag.so
    torch    the composition below: chain means, centred squares, between / within variance, the autocovariance at ALL lags by a
             zero-padded real FFT and its inverse, and Geyer's rule as a cumulative product of (P_k > 0) with a cumulative minimum
             -- float32 throughout, so its effective sample size differs from the launch's double sums in the last digits
             (``max_relative_difference`` of ess and rhat is printed, not asserted)

After `warmup` steps of every variant the variants alternate in `repeats` rounds of one block of `steps` steps each, so that
drift of the box hits both alike.  A block is timed with device events around the enqueued work, the figure is milliseconds per
step, and min / median / max over the blocks are reported with the torch / fused ratio at the medians.  A variant that runs out
of device memory is reported as such.  Nothing here is asserted by a test; bench.py is the project's yardstick and is not
involved.  Prints one JSON line per shape."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zhusuan-pytorch_amd"))

import torch  # noqa: E402

SHAPES = [(1000, 4, 10 ** 4), (1000, 4, 10 ** 6), (200, 20, 650000)]


def draws(T, C, E, dev):
    gen = torch.Generator(device=dev).manual_seed(T + C + E)
    phi = torch.linspace(-0.5, 0.9, E, device=dev)
    x = torch.empty(T, C, E, device=dev)
    x[0] = torch.randn(C, E, generator=gen, device=dev)
    for t in range(1, T):
        torch.addcmul(torch.randn(C, E, generator=gen, device=dev), phi, x[t - 1], out=x[t])
    x[:, C - 1] += 0.25
    return x


def torch_summary(x):
    """(mean, var+, rhat, ess) of x [T, C, E], split, no lag cap: the estimator of include/zs_diag.h with torch operations."""
    T = x.shape[0]
    N = T // 2
    X = torch.cat([x[:N], x[T - N:]], 1)          # [N, M, E]
    M = X.shape[1]
    mean_m = X.mean(0)
    d = X - mean_m
    W = (d.pow(2).sum(0) / (N - 1)).mean(0)
    varp = (N - 1) / N * W + mean_m.var(0, unbiased=True)
    rhat = (varp / W).sqrt()
    n_fft = 1 << (2 * N - 1).bit_length()
    f = torch.fft.rfft(d, n=n_fft, dim=0)
    acov = torch.fft.irfft(f.real.pow(2) + f.imag.pow(2), n=n_fft, dim=0)[:N] / N
    rho = 1 - (W - acov.mean(1)) / varp          # [N, E]
    L = N - N % 2
    P = rho[0:L:2] + rho[1:L:2]
    positive = (P > 0).to(P.dtype).cumprod(0)
    tau = -1 + 2 * (torch.cummin(P, 0).values * positive).sum(0)
    tau = tau.clamp(min=1 / math.log10(M * N))
    return mean_m.mean(0), varp, rhat, M * N / tau


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shapes", default="all", help="'all' or comma-separated indices into the shape list")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diag_kernel_bench needs a HIP device: there is nothing to time without one")
    import zhusuan.diagnostics as D
    dev = torch.device("cuda:0")
    shapes = SHAPES if args.shapes == "all" else [SHAPES[int(i)] for i in args.shapes.split(",")]
    for T, C, E in shapes:
        x = draws(T, C, E, dev)
        variants = [("fused", lambda: D.summary(x, chain_ndims=1)), ("torch", lambda: torch_summary(x))]
        results, failed = {}, {}
        for n, step in variants:
            try:
                for _ in range(args.warmup):
                    results[n] = step()
                torch.cuda.synchronize()
            except torch.cuda.OutOfMemoryError:
                failed[n] = "out of device memory"
                torch.cuda.empty_cache()
        out = dict(tool="diag_kernel_bench", T=T, C=C, E=E, split=True, dtype="float32", steps=args.steps, warmup=args.warmup,
                   repeats=args.repeats, device=torch.cuda.get_device_name(0), unit="ms_per_summary")
        if "fused" in results and "torch" in results:
            s, t = results["fused"], results["torch"]
            out["max_relative_difference"] = {"rhat": float("%.3g" % float(((s.rhat - t[2]) / t[2]).abs().max())),
                                              "ess": float("%.3g" % float(((s.ess - t[3]) / t[3]).abs().max()))}
            out["lags"] = {"mean": round(float(s.lags.float().mean()), 1), "max": int(s.lags.max())}
        results.clear()
        blocks = dict((n, []) for n, _ in variants if n not in failed)
        for _ in range(args.repeats):
            for n, step in variants:
                if n in failed:
                    continue
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.steps):
                    step()
                e1.record()
                torch.cuda.synchronize()
                blocks[n].append(e0.elapsed_time(e1) / args.steps)
        for n, _ in variants:
            if n in failed:
                out[n] = failed[n]
            else:
                b = blocks[n]
                out[n] = {"min": round(min(b), 3), "median": round(statistics.median(b), 3), "max": round(max(b), 3)}
        if not failed:
            out["torch_over_fused"] = round(out["torch"]["median"] / out["fused"]["median"], 2)
        print(json.dumps(out), flush=True)
        del x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
