"""Fixtures of the flow tests: runs of the REFERENCE's ``zhusuan.invertible``, ``FlowDistribution`` and ``ELBO(transform=)`` on CPU.

    python tests/golden/flow/gen_flow_golden.py [--ref /path/to/reference] [--out DIR]

Only imports and calls the reference; nothing of it is stored but data.  The models are those of tests/flow_models.py built on
the reference's classes, with seeded weights that are stored in the fixture (``w_<state_dict key>``).  Every case is run in
float32 and again in float64 on the same (float32-valued) weights and inputs; per quantity ``q`` the file holds the float32
result ``q`` and ``gap_q = max |q32 - q64|``: the reference's own rounding distance, which the tests' tolerance is built on.

  g_flow_layer_<kind>.npz   x, gy; forward: fwd_y, fwd_ld, fwd_gx, fwd_g_<param>; inverse: inv_y, inv_ld, inv_gx, inv_g_<param>
                            (gradients of sum(y * gy) + 0.7 * sum(log_det); MADE's inverse: values only, under no_grad)
  g_flow_nice.npz           x; lp = log_prob(x) [B], gx and g_<param> of -mean(lp)
  g_flow_elbo.npz           x, the standard-normal draws in call order (``torch.normal`` is wrapped in this process only, as in
                            tests/golden/mcmc/gen_mcmc_golden.py), loss and g_<param>"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import flow_models as M  # noqa: E402

_orig_normal = torch.normal


class Draws(object):
    """Recording (replay is None) or replaying wrapper of torch.normal."""

    def __init__(self, dtype, replay=None):
        self.dtype, self.replay, self.made = dtype, (list(replay) if replay is not None else None), []

    def __call__(self, mean, std=None, *, size=None, **kw):
        if size is not None:
            shape = tuple(size)
        else:
            shape = tuple(torch.broadcast_shapes(*[tuple(t.shape) for t in (mean, std) if isinstance(t, torch.Tensor)]))
        if self.replay is None:
            z = _orig_normal(0., 1., size=shape)
        else:
            z = torch.as_tensor(self.replay.pop(0))
            assert tuple(z.shape) == shape, (tuple(z.shape), shape)
        self.made.append(z.numpy().copy())
        return mean + std * z.to(self.dtype)


def npy(t):
    return t.detach().numpy().copy()


def weights_of(module):
    return {"w_" + k: npy(v) for k, v in module.state_dict().items()}


def grads_of(module, prefix):
    return {prefix + "g_" + k: npy(p.grad) for k, p in module.named_parameters() if p.grad is not None}


def run_layer(inv, kind, dtype, state=None):
    layer = M.make_layer(inv, kind)
    if state is None:
        M.randomize(layer, M.SEEDS[kind])
        state = {k: v.clone() for k, v in layer.state_dict().items()}
    else:
        layer.load_state_dict(state)
    layer = layer.to(dtype)
    x, gy = [torch.as_tensor(a, dtype=dtype) for a in M.layer_data(kind)]
    out = {}
    for prefix, reverse in (("fwd_", False), ("inv_", True)):
        for p in layer.parameters():
            p.grad = None
        values_only = kind == "made" and reverse          # the reference's inverse overwrites what its backward needs
        leaf = x.clone().requires_grad_(not values_only)
        if values_only:
            with torch.no_grad():
                y, ld = layer(leaf * 1.0, reverse=True)
        else:
            y, ld = layer(leaf * 1.0, reverse=reverse)
        out[prefix + "y"] = npy(y)
        if ld is not None:
            out[prefix + "ld"] = npy(ld)
        if values_only:
            continue
        loss = (y * gy).sum() + (M.LD_WEIGHT * ld.sum() if ld is not None else 0.0)
        loss.backward()
        out[prefix + "gx"] = npy(leaf.grad)
        out.update(grads_of(layer, prefix))
    return layer, state, out


def with_gaps(o32, o64):
    assert sorted(o32) == sorted(o64)
    res = dict(o32)
    for k in o32:
        res["gap_" + k] = np.float64(np.abs(o32[k].astype(np.float64) - o64[k]).max())
    return res


def generate(out_dir, ref_root):
    sys.path.insert(0, ref_root)
    for m in [k for k in sys.modules if k == "zhusuan" or k.startswith("zhusuan.")]:
        del sys.modules[m]
    import zhusuan.invertible as inv
    import zhusuan.distributions as dists
    from zhusuan.framework.bn import BayesianNet
    from zhusuan.variational.elbo import ELBO
    assert inv.__file__.startswith(ref_root), inv.__file__
    os.makedirs(out_dir, exist_ok=True)

    for kind in M.LAYERS:
        layer, state, o32 = run_layer(inv, kind, torch.float32)
        _, _, o64 = run_layer(inv, kind, torch.float64, state)
        x, gy = M.layer_data(kind)
        arrays = dict(with_gaps(o32, o64), x=x, gy=gy, **{"w_" + k: npy(v) for k, v in state.items()})
        np.savez(os.path.join(out_dir, "g_flow_layer_%s.npz" % kind), **arrays)
        print("%-14s %s" % (kind, " ".join("%s %.1e" % (k[4:], arrays[k]) for k in sorted(arrays) if k.startswith("gap_"))))

    # NICE log_prob
    def run_nice(dtype, state=None):
        net = M.make_nice(inv, dists, BayesianNet, dtype=dtype)
        if state is None:
            M.randomize(net, M.SEEDS["nice"])
            state = {k: v.clone() for k, v in net.state_dict().items()}
        else:
            net.load_state_dict(state)
        net = net.to(dtype)
        x = torch.as_tensor(nice_x, dtype=dtype).requires_grad_(True)
        lp = net(x * 1.0)
        (-lp.mean()).backward()
        return state, dict(lp=npy(lp), gx=npy(x.grad), **grads_of(net, ""))
    nice_x = np.random.RandomState(M.SEEDS["nice"]).uniform(size=(M.B, M.D)).astype(np.float32)
    state, o32 = run_nice(torch.float32)
    _, o64 = run_nice(torch.float64, state)
    arrays = dict(with_gaps(o32, o64), x=nice_x, **{"w_" + k: npy(v) for k, v in state.items()})
    np.savez(os.path.join(out_dir, "g_flow_nice.npz"), **arrays)
    print("%-14s %s" % ("nice", " ".join("%s %.1e" % (k[4:], arrays[k]) for k in sorted(arrays) if k.startswith("gap_"))))

    # ELBO(transform=)
    def run_elbo(dtype, state=None, replay=None):
        draws = Draws(dtype, replay)
        torch.normal = draws
        try:
            model = M.make_elbo(inv, dists, BayesianNet, ELBO, dtype=dtype)
            if state is None:
                M.randomize(model, M.SEEDS["elbo"])
                state = {k: v.clone() for k, v in model.state_dict().items()}
            else:
                model.load_state_dict(state)
            model = model.to(dtype)
            torch.manual_seed(M.SEEDS["elbo"])
            loss = model({'x': torch.as_tensor(elbo_x, dtype=dtype)})
            loss.backward()
        finally:
            torch.normal = _orig_normal
        return state, dict(loss=npy(loss), **grads_of(model, "")), draws.made
    elbo_x = (np.random.RandomState(M.SEEDS["elbo"]).uniform(size=(M.B, M.X_DIM)) < 0.5).astype(np.float32)
    state, o32, draws = run_elbo(torch.float32)
    _, o64, draws64 = run_elbo(torch.float64, state, replay=draws)
    assert len(draws) == len(draws64)
    arrays = dict(with_gaps(o32, o64), x=elbo_x, n_draws=np.int64(len(draws)), **{"w_" + k: npy(v) for k, v in state.items()})
    for i, z in enumerate(draws):
        arrays["draw_%02d" % i] = z
    np.savez(os.path.join(out_dir, "g_flow_elbo.npz"), **arrays)
    print("%-14s %d draws  %s" % ("elbo", len(draws), " ".join("%s %.1e" % (k[4:], arrays[k]) for k in sorted(arrays) if k.startswith("gap_"))))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    generate(a.out, a.ref)
