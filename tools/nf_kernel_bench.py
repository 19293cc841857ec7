#!/usr/bin/env python
"""The planar and Householder flow stacks of ``zhusuan.transform`` (include/zs_nf.h), forward + backward, against the plain torch
modules of examples/flow_vae.py, eager, on the same GPU, in the same process and on the same parameters and inputs.

    python tools/nf_kernel_bench.py [--steps 50] [--warmup 10] [--repeats 7]

Shapes: D = 40, B in {64, 512, 4096}; planar stacks of L in {1, 8, 32} layers, Householder stacks of L in {5, 32} reflections whose
vectors come from the chain of linear layers (500 -> 40, then 40 -> 40) on both sides.

    fused    PlanarFlow / HouseholderFlow: one launch of libzs_nf.so forward; backward one launch, plus the small finish of the
             parameter gradients for the planar stack (the linear chain and the stacking of its outputs are torch's on both sides)
    torch    the example's PF layers applied in a loop with the log-dets summed / the example's HouseHolderFlow

A step evaluates ``sum(z_out) + sum(log_det)``, backpropagates it into z and every parameter.  After `warmup` steps of every
variant the variants alternate in `repeats` rounds of one block of `steps` steps each, so that drift of the box hits both alike.
A block is timed with device events around the enqueued work (kernels and the gaps between them), the figure is microseconds per
step, and min / median / max over the blocks are reported with the torch / fused ratio at the medians.  These are times of whole
launch-bound Python steps; the kernels' own durations are not measured here.  ``ops`` is the number of ATen operations one step
dispatches (forward and backward; every one that is not a view is at least one launch) and ``nf_launches`` the launches of
libzs_nf.so among the fused side's.  Nothing here is asserted by a test; bench.py is the project's yardstick and is not involved.
Prints one JSON line per case."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zhusuan-pytorch_amd"))

import torch  # noqa: E402
from torch.utils._python_dispatch import TorchDispatchMode  # noqa: E402

D, V = 40, 500
BATCHES = [64, 512, 4096]
CASES = [("planar", L) for L in (1, 8, 32)] + [("householder", L) for L in (5, 32)]


class CountOps(TorchDispatchMode):
    def __init__(self):
        super(CountOps, self).__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


def cases(kind, L, B, dev):
    import zhusuan as zs
    from examples import flow_vae
    gen = torch.Generator().manual_seed(B + L)
    z = torch.randn(B, D, generator=gen).to(dev).requires_grad_(True)
    if kind == "planar":
        torch.manual_seed(L)
        fused_mod = zs.PlanarFlow(D, L).to(dev)
        with torch.no_grad():          # rand's all-positive vectors make w.u about D / 4: centre them
            fused_mod.u.sub_(0.5)
            fused_mod.w.sub_(0.5)
        layers = [flow_vae.PF(D).to(dev) for _ in range(L)]
        with torch.no_grad():
            for l, pf in enumerate(layers):
                pf.u.copy_(fused_mod.u[l:l + 1]), pf.w.copy_(fused_mod.w[l:l + 1]), pf.b.copy_(fused_mod.b[l:l + 1])

        def fused():
            out, ld = fused_mod(z)
            (out.sum() + ld.sum()).backward()

        def eager():
            out, total = z, 0.0
            for pf in layers:
                out, ld = pf(out)
                total = total + ld
            (out.sum() + total.sum()).backward()
        leaves = [z] + list(fused_mod.parameters()), [z] + [p for pf in layers for p in pf.parameters()]
    else:
        aux = torch.randn(B, V, generator=gen).to(dev)
        torch.manual_seed(L)
        fused_mod = zs.HouseholderFlow(D, V, L).to(dev)
        torch_mod = flow_vae.HouseHolderFlow(D, V, L).to(dev)
        with torch.no_grad():
            for mine, hf in zip(fused_mod.v_layers, torch_mod.flow.layers):
                hf.v_layer.weight.copy_(mine.weight), hf.v_layer.bias.copy_(mine.bias)

        def fused():
            out, _ = fused_mod((z, aux))
            out.sum().backward()

        def eager():
            out, _ = torch_mod.forward((z, aux))
            out["z"].sum().backward()
        leaves = [z] + list(fused_mod.parameters()), [z] + list(torch_mod.parameters())
    return leaves, fused, eager


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("nf_kernel_bench needs a HIP device: there is nothing to time without one")
    dev = torch.device("cuda:0")
    from zhusuan import _nf_hip
    launches = [0]

    def counted(fn):
        def call(*a, **k):
            launches[0] += 1
            return fn(*a, **k)
        return call
    for name in ("planar_fwd", "planar_bwd", "planar_finish", "householder_fwd", "householder_bwd"):
        setattr(_nf_hip, name, counted(getattr(_nf_hip, name)))
    for kind, L in CASES:
        for B in BATCHES:
            (lf, lt), fused, eager = cases(kind, L, B, dev)
            variants = [("fused", fused, lf), ("torch", eager, lt)]
            zgrad, ops = {}, {}
            for n, step, leaves in variants:
                for _ in range(args.warmup):
                    for t in leaves:
                        t.grad = None
                    step()
                zgrad[n] = leaves[0].grad.clone()
                for t in leaves:
                    t.grad = None
                launches[0] = 0
                with CountOps() as c:
                    step()
                ops[n] = c.n
                if n == "fused":
                    nf_launches = launches[0]
            torch.cuda.synchronize()
            diff = float((zgrad["fused"] - zgrad["torch"]).abs().max()) / max(float(zgrad["torch"].abs().max()), 1e-30)
            blocks = dict((n, []) for n, _, _ in variants)
            for _ in range(args.repeats):
                for n, step, leaves in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.steps):
                        for t in leaves:
                            t.grad = None
                        step()
                    e1.record()
                    torch.cuda.synchronize()
                    blocks[n].append(e0.elapsed_time(e1) * 1e3 / args.steps)
            out = dict(tool="nf_kernel_bench", flow=kind, L=L, B=B, D=D, steps=args.steps, warmup=args.warmup, repeats=args.repeats,
                       device=torch.cuda.get_device_name(0), unit="us_per_forward_plus_backward",
                       max_dz_difference_relative=float("%.3g" % diff), nf_launches=nf_launches)
            for n, _, _ in variants:
                b = blocks[n]
                out[n] = {"ops": ops[n], "min": round(min(b), 1), "median": round(statistics.median(b), 1), "max": round(max(b), 1)}
            out["torch_over_fused"] = round(out["torch"]["median"] / out["fused"]["median"], 2)
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
