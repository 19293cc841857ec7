"""TEST INFRASTRUCTURE, companion of tests/hmc_host.py for the categorical families: ``install()`` replaces the functions of the
binding (``zhusuan._cat_hip.sample_logprob`` ... ``relaxed_logprob_bwd``) by torch restatements of the kernel contract of
include/zs_cat.h on CPU tensors, so that the host logic of the distributions (shapes, broadcasting, caching, autograd wiring,
draw order, call ids, launch budget) runs on a GPU-less machine.  The package itself contains no such routing.

The restatements evaluate the header's formulas in float64 and round the results to the tensors' dtype.  Where no noise is
injected, the uniforms are flat elements of the C oracle's ``zs_philox_uniform_f32`` stream for the launch's (seed, call): the
kernels' noise contract.  ``recording()`` lists every launch (tests/host_routing.py).

``reference_*`` are the same formulas in pure float64 on float64 inputs, written with torch's own ``logsumexp`` / autograd: the
truth of the kernel and distribution tests."""
import math

import torch

import host_routing

F64 = torch.float64


def philox_uniform(n, seed, call, rng_state=None):
    return host_routing.philox("zs_philox_uniform_f32", n, seed, call, rng_state)


# ------------------------------------------------------------------------------------------------ the float64 truth
def reference_perturbed(logits, u):
    """v[k,r,j] = logits[r,j] - log(-log u[k,r,j])"""
    return logits.to(F64)[None] - torch.log(-torch.log(u.to(F64)))


def reference_logprob_index(logits, idx):
    """lp[k,r] = logits[r, idx[k,r]] - lse_r ; NaN for an index outside [0, N).  idx [K, R]."""
    lg = logits.to(F64)
    N = lg.shape[1]
    ok = (idx >= 0) & (idx < N)
    picked = torch.gather(lg[None].expand(idx.shape[0], -1, -1), 2, idx.clamp(0, N - 1)[..., None])[..., 0]
    lp = picked - torch.logsumexp(lg, dim=1)[None]
    return torch.where(ok, lp, torch.full_like(lp, float("nan")))


def reference_logprob_weights(logits, x):
    """lp[k,r] = sum_j x l - (sum_j x) lse, a term with x == 0 exactly 0.  x [K, R, N]."""
    lg = logits.to(F64)[None]
    x = x.to(F64)
    terms = torch.where(x == 0, torch.zeros_like(x), x * lg)
    return terms.sum(-1) - x.sum(-1) * torch.logsumexp(lg, dim=-1)


def reference_sample(logits, u):
    """(idx [K, R], lp [K, R], v [K, R, N]) of the Gumbel-max draw; ties to the lowest index."""
    v = reference_perturbed(logits, u)
    N = v.shape[-1]
    top = v.max(dim=-1, keepdim=True).values
    first = torch.where(v == top, torch.arange(N).expand_as(v), torch.full_like(v, N, dtype=torch.int64))
    idx = first.min(dim=-1).values.clamp(max=N - 1)
    return idx, reference_logprob_index(logits, idx), v


def relaxed_c0(N, tau):
    return math.lgamma(N) + (N - 1) * math.log(tau)


def reference_relaxed_logprob(logits, y, tau, exp_space):
    """lp = lgamma(N) + (N - 1) log tau + sum t - N lse(t) [- sum y],  t = logits - tau y.  y [K, R, N]."""
    lg = logits.to(F64)[None]
    y = y.to(F64)
    N = lg.shape[-1]
    t = lg - tau * y
    lp = relaxed_c0(N, tau) + t.sum(-1) - N * torch.logsumexp(t, dim=-1)
    return lp - y.sum(-1) if exp_space else lp


def reference_relaxed_y(logits, u, tau):
    a = reference_perturbed(logits, u) / tau
    return a - torch.logsumexp(a, dim=-1, keepdim=True)


def reference_relaxed(logits, u, tau, exp_space):
    """(y, lp) of the relaxed draw."""
    y = reference_relaxed_y(logits, u, tau)
    return y, reference_relaxed_logprob(logits, y, tau, exp_space)


# ------------------------------------------------------------------------------------------------ the routed binding
def _uniforms(logits, K, u, seed, call, rng_state):
    R, N = logits.shape
    if u is not None:
        return u.reshape(K, R, N)
    return philox_uniform(K * R * N, seed, call, rng_state).reshape(K, R, N)


def sample_logprob(logits, K, u=None, seed=0, call=0, rng_state=None, want_index=True, want_onehot=False):
    host_routing.host_only("cat_host", [logits, u, rng_state])
    R, N = logits.shape
    with torch.no_grad():
        idx, lp, _ = reference_sample(logits, _uniforms(logits, K, u, seed, call, rng_state))
        onehot = torch.nn.functional.one_hot(idx, N).to(logits.dtype) if want_onehot else None
    return (idx if want_index else None), onehot, lp.to(logits.dtype)


def _rows(v, K, R, event):
    return v.reshape((-1, R) + event).expand((K, R) + event)


def logprob(logits, K, idx=None, x=None):
    host_routing.host_only("cat_host", [logits, idx, x])
    R, N = logits.shape
    with torch.no_grad():
        if x is None:
            return reference_logprob_index(logits, _rows(idx, K, R, ())).to(logits.dtype)
        return reference_logprob_weights(logits, _rows(x, K, R, (N,))).to(logits.dtype)


def logprob_bwd(logits, K, glp, idx=None, x=None, want_gx=False):
    host_routing.host_only("cat_host", [logits, idx, x, glp])
    R, N = logits.shape
    with torch.no_grad():
        lg, g = logits.to(F64), glp.to(F64).reshape(K, R)
        if x is None:
            i = _rows(idx, K, R, ())
            ok = (i >= 0) & (i < N)
            xx = torch.nn.functional.one_hot(i.clamp(0, N - 1), N).to(F64) * ok[..., None]
        else:
            xx = _rows(x, K, R, (N,)).to(F64)
        sm = torch.softmax(lg, dim=1)
        glogits = (g[..., None] * xx).sum(0) - (g * xx.sum(-1)).sum(0)[:, None] * sm
        gx = None
        if want_gx:
            gx = (g[..., None] * (lg - torch.logsumexp(lg, dim=1, keepdim=True))[None]).to(logits.dtype)
    return glogits.to(logits.dtype), gx


def relaxed_sample_logprob(logits, K, tau, exp_space, u=None, seed=0, call=0, rng_state=None):
    host_routing.host_only("cat_host", [logits, u, rng_state])
    with torch.no_grad():
        y, lp = reference_relaxed(logits, _uniforms(logits, K, u, seed, call, rng_state), tau, exp_space)
    return y.to(logits.dtype), (torch.exp(y).to(logits.dtype) if exp_space else None), lp.to(logits.dtype)


def _q(logits, y, tau):
    t = logits.to(F64)[None] - tau * y.to(F64)
    return 1.0 - logits.shape[1] * torch.softmax(t, dim=-1)


def relaxed_sample_logprob_bwd(logits, K, tau, exp_space, y, gy=None, gey=None, glp=None):
    host_routing.host_only("cat_host", [logits, y, gy, gey, glp])
    R, N = logits.shape
    e = 1.0 if exp_space else 0.0
    with torch.no_grad():
        yy = y.to(F64).reshape(K, R, N)
        q = _q(logits, yy, tau)
        g = torch.zeros(K, R, dtype=F64) if glp is None else glp.to(F64).reshape(K, R)
        G = g[..., None] * (-tau * q - e)
        if gy is not None:
            G = G + gy.to(F64).reshape(K, R, N)
        if gey is not None and exp_space:
            G = G + gey.to(F64).reshape(K, R, N) * torch.exp(yy)
        glogits = ((G - torch.exp(yy) * G.sum(-1, keepdim=True)) / tau + g[..., None] * q).sum(0)
    return glogits.to(logits.dtype)


def relaxed_logprob(logits, K, tau, exp_space, y):
    host_routing.host_only("cat_host", [logits, y])
    R, N = logits.shape
    with torch.no_grad():
        return reference_relaxed_logprob(logits, _rows(y, K, R, (N,)), tau, exp_space).to(logits.dtype)


def relaxed_logprob_bwd(logits, K, tau, exp_space, y, glp, want_gy=True, want_glogits=True):
    host_routing.host_only("cat_host", [logits, y, glp])
    R, N = logits.shape
    e = 1.0 if exp_space else 0.0
    with torch.no_grad():
        q = _q(logits, _rows(y, K, R, (N,)), tau)
        g = glp.to(F64).reshape(K, R)[..., None]
        gy = (g * (-tau * q - e)).to(logits.dtype) if want_gy else None
        glogits = (g * q).sum(0).to(logits.dtype) if want_glogits else None
    return gy, glogits


router = host_routing.Router("zhusuan._cat_hip", {
    "sample_logprob": sample_logprob, "logprob": logprob, "logprob_bwd": logprob_bwd,
    "relaxed_sample_logprob": relaxed_sample_logprob, "relaxed_sample_logprob_bwd": relaxed_sample_logprob_bwd,
    "relaxed_logprob": relaxed_logprob, "relaxed_logprob_bwd": relaxed_logprob_bwd})
install, uninstall, recording = router.install, router.uninstall, router.recording
# the suite's ``dev`` fixture (host and hip) with the categorical binding routed accordingly: imported by the tests
cdev = host_routing.dev_fixture("cdev", router)
