"""TEST INFRASTRUCTURE, companion of tests/mvn_host.py for the inclusive-KL objective: ``install()`` replaces the two functions of
the binding (``zhusuan._klpq_hip.forward`` / ``backward``) by torch restatements of the kernel contract of include/zs_klpq.h on
CPU tensors, so that the host logic of the objective (layouts, term tables, autograd wiring, launch budget) runs on a GPU-less
machine.  The package itself contains no such routing.

The restatements evaluate the header's formulas in float64 and round the results to the tensors' dtype.  ``recording()`` lists
every launch (tests/host_routing.py).  ``reference_*`` are the same formulas in pure float64 on float64 inputs: the truth of the kernel and objective tests."""
import math

import torch

import host_routing

F64 = torch.float64


# ------------------------------------------------------------------------------------------------ the float64 truth
def side_sum(terms, K, B):
    """The side's [K, B] log-probability: the terms (each broadcastable to [K, B]) added left to right, in float64."""
    total = None
    for t in terms:
        t = t.to(F64).expand(K, B)
        total = t if total is None else total + t
    return total


def reference_forward(terms_p, terms_q, K, B, model_grad=False):
    """dict(lp, lq, lw [K, B]; w [B, K]; cost, bound, ess [B]; mean []) of Q1."""
    lp, lq = side_sum(terms_p, K, B), side_sum(terms_q, K, B)
    lw = lp - lq
    m = lw.max(0, keepdim=True).values
    e = torch.exp(lw - m)
    s = e.sum(0, keepdim=True)
    w = e / s
    x = lq + lp if model_grad else lq
    cost = -torch.where(w == 0, torch.zeros_like(w), w * x).sum(0)
    bound = (m + torch.log(s))[0] - math.log(K)
    return dict(lp=lp, lq=lq, lw=lw, w=w.t().contiguous(), cost=cost, bound=bound, ess=1.0 / (w * w).sum(0), mean=cost.mean())


def reference_backward(w, gcost, gbound, model_grad, B, gcost_is_mean=False):
    """(gq, gp), each [K, B]: what every variational and every generator term receives, before any broadcast sum."""
    w = w.to(F64).t()
    gc = (gcost.to(F64).reshape(()) / B).expand(B) if gcost_is_mean else gcost.to(F64)
    gb = torch.zeros(B, dtype=F64) if gbound is None else gbound.to(F64)
    gq = -gc[None] * w - gb[None] * w
    gp = (-gc[None] * w + gb[None] * w) if model_grad else gb[None] * w
    return gq, gp


def reduce_to(g, shape):
    """A [K, B] gradient summed over the axes along which a term of ``shape`` is shared."""
    for d in (0, 1):
        if shape[d] == 1 and g.shape[d] != 1:
            g = g.sum(d, keepdim=True)
    return g


# ------------------------------------------------------------------------------------------------ the routed binding
def forward(terms_p, terms_q, K, B, model_grad=False, bound_only=False, want_mean=False):
    host_routing.host_only("klpq_host", list(terms_p) + list(terms_q))
    dtype = terms_q[0].dtype
    with torch.no_grad():
        r = reference_forward(terms_p, terms_q, K, B, model_grad)
    if bound_only:
        return None, None, r["bound"].to(dtype), None, None
    assert not want_mean or B <= 1024
    return r["w"].to(dtype), r["cost"].to(dtype), r["bound"].to(dtype), r["ess"].to(dtype), (r["mean"].to(dtype) if want_mean else None)


def backward(layouts_p, layouts_q, want_p, want_q, K, B, w, gcost, gbound=None, model_grad=False, gcost_is_mean=False):
    host_routing.host_only("klpq_host", [w, gcost, gbound])
    with torch.no_grad():
        gq, gp = reference_backward(w, gcost, gbound, model_grad, B, gcost_is_mean)

        def give(lay, want, g):
            if not want:
                return None
            (k, b), (sk, sb) = lay
            out = torch.empty_strided((k, b), (sk or 1, sb or 1), dtype=w.dtype)
            out.copy_(reduce_to(g, (k, b)))
            return out
        return ([give(lay, wnt, gp) for lay, wnt in zip(layouts_p, want_p)], [give(lay, wnt, gq) for lay, wnt in zip(layouts_q, want_q)])


router = host_routing.Router("zhusuan._klpq_hip", {"forward": forward, "backward": backward})
install, uninstall, recording = router.install, router.uninstall, router.recording
# the suite's ``dev`` fixture (host and hip) with the inclusive-KL binding routed accordingly: imported by the tests
kdev = host_routing.dev_fixture("kdev", router)
