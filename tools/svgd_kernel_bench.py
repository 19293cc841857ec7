#!/usr/bin/env python
"""One SVGD step over K particles of D dimensions (include/zs_svgd.h: gram, finish, update on the matrix-core kernels) against the
torch composition of the same formulas (zhusuan.mcmc.SVGD.torch_step) on the same GPU and the same operands.

    python tools/svgd_kernel_bench.py [--steps 20] [--warmup 5] [--repeats 5] [--limit 240]

Shapes: K in {16, 64, 256}, D in {10^3, 10^5, 10^6}, float32, one latent, the median rule, the plain step.  Five measurements a
shape: each of the three launches on its own, the three in a row ("fused"), and the composition ("torch": mean, sub, matmul,
quantile, exp, two more matmul and the step).  The gradient of the log density is an operand here, not part of the step.

After `warmup` steps of every variant the variants alternate in `repeats` rounds of one block of `steps` steps each, so that
drift of the box hits all alike.  A block is timed with device events around the enqueued work; the figure is milliseconds per
step, min / median / max over the blocks, with the torch / fused ratio at the medians.  Every shape runs in a child process of its
own under a time limit (`--limit` seconds), and the first one that fails ends the run.  The JSON lines go to stdout and to
profiles/svgd_kernel_bench.txt.  Nothing here is asserted by a test; bench.py is the project's yardstick and is not involved."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zhusuan-pytorch_amd"))

PARTICLES = [16, 64, 256]
DIMS = [10 ** 3, 10 ** 5, 10 ** 6]


def one(K, D, args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("svgd_kernel_bench needs a HIP device: there is nothing to time without one")
    from zhusuan import _svgd_hip as B
    from zhusuan.mcmc.SVGD import torch_step
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1000 * K + D % 997)
    q = torch.randn(K, D, generator=gen, device=dev)
    g = torch.randn(K, D, generator=gen, device=dev)
    out = torch.empty_like(q)
    slots = B.slots(D)
    partials = torch.empty(slots * K * K, dtype=torch.float64, device=dev)
    state = torch.empty(B.state_doubles(K), dtype=torch.float64, device=dev)

    def gram():
        B.gram(K, [q], partials)

    def finish():
        B.finish(K, partials, slots, state)

    def update():
        B.update(K, [q], [g], [out], state, 1e-3)

    def fused():
        gram(), finish(), update()

    def composed():
        phis, _, _ = torch_step([q], [g])
        torch.add(q, phis[0], alpha=1e-3, out=out)

    variants = [("gram", gram), ("finish", finish), ("update", update), ("fused", fused), ("torch", composed)]
    fused()
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
    res = dict(tool="svgd_kernel_bench", K=K, D=D, dtype="float32", slots=slots, steps=args.steps, warmup=args.warmup,
               repeats=args.repeats, device=torch.cuda.get_device_name(0), unit="ms_per_step")
    for name, _ in variants:
        b = blocks[name]
        res[name] = {"min": round(min(b), 4), "median": round(statistics.median(b), 4), "max": round(max(b), 4)}
    res["torch_over_fused"] = round(res["torch"]["median"] / res["fused"]["median"], 2)
    print(json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240)
    ap.add_argument("--one", type=int, nargs=2, metavar=("K", "D"), help="time this shape in this process")
    args = ap.parse_args()
    if args.one:
        return one(args.one[0], args.one[1], args)
    lines = []
    for K in PARTICLES:
        for D in DIMS:
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--one", str(K), str(D),
                   "--steps", str(args.steps), "--warmup", str(args.warmup), "--repeats", str(args.repeats)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                sys.stderr.write(r.stdout + r.stderr)
                raise SystemExit("svgd_kernel_bench: K = %d, D = %d ended with status %d; nothing more is started" % (K, D, r.returncode))
            print(r.stdout, end="", flush=True)
            lines.append(r.stdout)
    with open(os.path.join(ROOT, "profiles", "svgd_kernel_bench.txt"), "w") as f:
        f.write("".join(lines))


if __name__ == "__main__":
    main()
