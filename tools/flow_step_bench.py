#!/usr/bin/env python
"""A training step of the two flow examples at the reference's sizes, flow kernels against the reference's op sequence.

    python tools/flow_step_bench.py [--steps 200] [--warmup 30] [--repeats 5] [--only vae|nice] [--no-graph]

Workloads (forward, backward and a torch.optim.Adam step each):

    vae    examples/flow_vae.py, NICE transform: B = 64, x = 784, z = 40, hidden 500, ten couplings of four layers (hidden 64)
           and a scaling between q and p (examples/normlizing_flows/flow_vae.py:179-195 of the reference)
    nice   examples/nice.py: B = 200, D = 784, hidden 1000, four couplings of five layers and a scaling under a Logistic base
           (examples/normlizing_flows/nice_mnist.py:42-50)

Variants, on the same GPU, same weights, same data:

    fused  zhusuan.invertible / FlowDistribution: split, merge, scaling and the log-density tail are one launch each way
    torch  the same model with the flow layers written as the reference writes them, op by op in plain torch (mask multiplies,
           1 - mask, masked shift, adds; exp, in-place multiply, sum; log-density, row sum, add), everything else identical

each launched eagerly (`fused`, `torch`) and replayed as one hipGraph (`fused_graph`, `torch_graph`: `zhusuan.GraphedStep` around the
same step with a capturable Adam; a variant whose capture fails is reported as an error string, the others still run).

Before anything is timed the two variants are evaluated once on the same weights, data and draws and the relative difference of
their losses is recorded (`loss_rel_diff`), and the flow-kernel launches of one fused step are counted by wrapping the
`_flow_hip` functions for that one step only: nothing is wrapped while the clock runs.  After `warmup` steps of every variant the
variants alternate in `repeats` rounds of one block of `steps` steps each, so that drift of the box hits all alike.  A block is
timed on the host around a device synchronisation (a block of 200 eager steps is 0.5 to 1.5 s, of 200 replays 0.1 to 0.4 s);
the figure is microseconds per step, and min / median / max over the blocks are reported.  Nothing here is asserted by a test;
bench.py is the project's yardstick and is not involved.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zhusuan-pytorch_amd"))

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402


def torch_layers():
    """The reference's MaskCoupling and Scaling op sequences (coupling.py:65-75, scaling.py:26-34) as plain torch modules."""
    from zhusuan.invertible import RevNet

    class TorchMaskCoupling(RevNet):
        """Seven element-wise launches around the inner network, as there: mask * x, 1 - mask, its product with x, 1 - mask again,
        its product with the shift, the add (or subtract) and the final add."""

        def __init__(self, fused):
            super().__init__()
            self.nn, self.mask = fused.nn, fused.mask          # the SAME inner network (shared parameters)

        def _couple(self, x, reverse):
            kept = self.mask * x
            moved = (1. - self.mask) * x
            delta = self.nn(kept) * (1. - self.mask)
            moved = moved - delta if reverse else moved + delta
            return kept + moved, None

        def _forward(self, x, **kw):
            return self._couple(x, False)

        def _inverse(self, y, **kw):
            return self._couple(y, True)

    class TorchScaling(RevNet):
        """A sum, an exp (a negation first when inverting) and an in-place multiply, as there."""

        def __init__(self, fused):
            super().__init__()
            self.log_scale = fused.log_scale

        def _forward(self, x, **kw):
            total = self.log_scale.sum()
            return x.mul_(self.log_scale.exp()), total

        def _inverse(self, y, **kw):
            total = self.log_scale.sum()
            return y.mul_(torch.exp(-self.log_scale)), total
    return TorchMaskCoupling, TorchScaling


def torch_twin(flow):
    """A RevSequential over the same parameters whose layers are the plain-torch restatements."""
    from zhusuan.invertible import RevSequential, MaskCoupling
    TM, TS = torch_layers()
    return RevSequential([TM(f) if isinstance(f, MaskCoupling) else TS(f) for f in flow.layers])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default=None, choices=["vae", "nice"])
    ap.add_argument("--no-graph", action="store_true", help="time the eagerly launched variants only")
    args = ap.parse_args()

    import copy
    import zhusuan as zs
    from zhusuan import _flow_hip
    from examples import flow_vae, nice
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    torch.cuda.manual_seed(0)
    g = torch.Generator().manual_seed(1)
    KERNELS = ("split", "split_bwd", "merge", "merge_bwd", "scale_fwd", "scale_bwd", "tail", "tail_bwd")

    def count_launches(step):
        """Flow-kernel launches of ONE call of `step` (the wrappers are removed again before anything is timed)."""
        n, saved = [0], {name: getattr(_flow_hip, name) for name in KERNELS}

        def counted(f):
            def call(*a, **k):
                n[0] += 1
                return f(*a, **k)
            return call
        for name, f in saved.items():
            setattr(_flow_hip, name, counted(f))
        try:
            step()
        finally:
            for name, f in saved.items():
                setattr(_flow_hip, name, f)
        return n[0]

    def eager(params, loss_of):
        params = list(params)
        opt = torch.optim.Adam(params, lr=1e-3)

        def step():
            opt.zero_grad()
            loss = loss_of()
            loss.backward()
            opt.step()
        return step

    def graphed(params, loss_of, draws):
        params = list(params)
        opt = torch.optim.Adam(params, lr=1e-3, capturable=True)
        rng = zs.DeviceRNG(dev, seed=0) if draws else None

        def compute():
            if rng is not None:
                rng.begin_step()
            for p in params:
                p.grad = None
            loss = loss_of()
            loss.backward()
            return loss.detach()
        return zs.GraphedStep(compute, opt.step, rng=rng, warmup=3)

    def rel_diff(a, b):
        return abs(float(a) - float(b)) / max(abs(float(b)), 1e-30)

    def vae_variants():
        x = {"x": (torch.rand(64, 784, generator=g) < 0.5).float().to(dev)}

        def pair():
            fused = flow_vae.build("NICE", 64, device=dev)
            twin = copy.deepcopy(fused)
            twin.transform.flow = torch_twin(twin.transform.flow)
            return fused, twin
        fused, twin = pair()
        eps = [torch.randn(64, 40, generator=g).to(dev) for _ in range(2)]
        with torch.no_grad():
            with zs.inject_epsilon(eps):
                lf = fused(x)
            with zs.inject_epsilon(eps):
                lt = twin(x)
        gf, gt = pair()
        return rel_diff(lf, lt), [("fused", lambda: eager(fused.parameters(), lambda: fused(x))),
                                  ("torch", lambda: eager(twin.parameters(), lambda: twin(x))),
                                  ("fused_graph", lambda: graphed(gf.parameters(), lambda: gf(x), True)),
                                  ("torch_graph", lambda: graphed(gt.parameters(), lambda: gt(x), True))]

    def nice_variants():
        x = torch.rand(200, 784, generator=g).to(dev)

        def pair():
            fused = nice.build(device=dev)
            twin = copy.deepcopy(fused)
            flow, dis = torch_twin(twin.flow), twin.nodes["x"].dist.latents

            def twin_loss():
                z, log_det = flow(x * 1.0)
                return -(torch.sum(dis.log_prob(z), dim=1) + log_det).mean()          # flow_distribution.py:49-51
            return fused, (lambda: -fused(x * 1.0).mean()), flow, twin_loss
        fused, fused_loss, flow, twin_loss = pair()
        with torch.no_grad():
            diff = rel_diff(fused_loss(), twin_loss())
        gfused, gfused_loss, gflow, gtwin_loss = pair()
        return diff, [("fused", lambda: eager(fused.parameters(), fused_loss)), ("torch", lambda: eager(flow.parameters(), twin_loss)),
                      ("fused_graph", lambda: graphed(gfused.parameters(), gfused_loss, False)),
                      ("torch_graph", lambda: graphed(gflow.parameters(), gtwin_loss, False))]

    out = {"tool": "flow_step_bench", "steps": args.steps, "warmup": args.warmup, "repeats": args.repeats,
           "device": torch.cuda.get_device_name(0), "unit": "us_per_step"}
    for wname, make in (("vae", vae_variants), ("nice", nice_variants)):
        if args.only and args.only != wname:
            continue
        diff, makers = make()
        res = {"loss_rel_diff": diff}
        variants = []
        for name, maker in makers:
            if "graph" in name and args.no_graph:
                continue
            try:
                variants.append((name, maker()))
            except Exception as e:          # noqa: BLE001  (a failed capture: reported, the other variants still run)
                res[name] = {"error": repr(e)[:300]}
        res["flow_kernel_launches_per_step"] = count_launches(dict(variants)["fused"])
        for _, step in variants:
            for _ in range(args.warmup):
                step()
        torch.cuda.synchronize()
        blocks = dict((name, []) for name, _ in variants)
        for _ in range(args.repeats):          # the variants alternate block by block: drift of the box hits all alike
            for name, step in variants:
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    step()
                torch.cuda.synchronize()
                blocks[name].append((time.perf_counter() - t0) * 1e6 / args.steps)
        for name, _ in variants:
            b = blocks[name]
            res[name] = {"min": round(min(b), 1), "median": round(statistics.median(b), 1), "max": round(max(b), 1)}
        out[wname] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
