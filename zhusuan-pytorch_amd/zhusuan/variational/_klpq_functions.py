"""The autograd Function of the inclusive-KL objective over the kernels of include/zs_klpq.h (``zhusuan._klpq_hip``, looked up at
call time): Q1 forward in one launch, its backward in one more.  Nothing here synchronises with the host, so an objective step
captures inside ``GraphedStep``."""
import torch
from torch.autograd.function import once_differentiable

from .. import _klpq_hip


def kernel_term(t, K, B):
    """A log-probability tensor as a term of the launch: a 2-D ``[K or 1, B or 1]`` tensor that the kernel addresses by its two
    strides -- ``[K, B]``-contiguous, a transposed ``[B, K]``-contiguous view and size-1 axes enter as they are; anything else
    (a slice with gaps) is made contiguous first."""
    if not (t.is_contiguous() or t.t().is_contiguous()):
        t = t.contiguous()
    return t


class InclusiveKL(torch.autograd.Function):
    """``(cost, bound, ess)`` of Q1.  ``cost`` is ``[B]``, or the batch mean (a scalar) with ``want_mean``; ``bound`` (the
    importance-weighted bound per datapoint, detached: upstream's klpq never differentiates it) and ``ess`` are ``[B]``.  The
    weights are constants in the backward: every variational term receives ``-gcost w``, and with ``model_grad`` so does every
    generator term.  The first ``n_p`` of ``terms`` are the generator's."""

    @staticmethod
    def forward(ctx, K, B, n_p, model_grad, want_mean, *terms):
        terms_p, terms_q = list(terms[:n_p]), list(terms[n_p:])
        in_launch = want_mean and B <= _klpq_hip.MEAN_MAX_BATCH
        w, cost, bound, ess, mean = _klpq_hip.forward(terms_p, terms_q, K, B, model_grad=model_grad, want_mean=in_launch)
        ctx.set_materialize_grads(False)          # an output that did not enter the loss brings None, not zeros
        ctx.meta = (K, B, n_p, model_grad, want_mean, [_klpq_hip.layout(t) for t in terms])
        ctx.save_for_backward(w)          # (of the terms the backward needs the layouts only)
        ctx.mark_non_differentiable(bound, ess)
        if want_mean:
            cost = mean if in_launch else cost.mean()          # beyond the one-workgroup batch the mean is torch's
        return cost, bound, ess

    @staticmethod
    @once_differentiable
    def backward(ctx, gcost, _gbound, _gess):
        K, B, n_p, model_grad, want_mean, layouts = ctx.meta
        w, = ctx.saved_tensors
        need = ctx.needs_input_grad[5:]
        want_p = [bool(n) and model_grad for n in need[:n_p]]
        want_q = [bool(n) for n in need[n_p:]]
        none = (None,) * 5
        if gcost is None or not (any(want_p) or any(want_q)):
            return none + (None,) * len(layouts)
        gcost = gcost.contiguous()
        gp, gq = _klpq_hip.backward(layouts[:n_p], layouts[n_p:], want_p, want_q, K, B, w, gcost, model_grad=model_grad,
                                    gcost_is_mean=want_mean)
        return none + tuple(gp) + tuple(gq)
