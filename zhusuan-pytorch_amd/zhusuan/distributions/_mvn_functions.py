"""Autograd Functions of MultivariateNormalCholesky over the kernels of include/zs_mvn.h (``zhusuan._mvn_hip``, looked up at call
time).  ``mean`` is always the contiguous ``[R, D]`` view and ``tril`` the contiguous ``[R, D, D]`` one, per-particle operands are
``[K, R(, D)]``; one launch forward, one launch backward."""
import torch
from torch.autograd.function import once_differentiable

from .. import _mvn_hip


def _dense(g, shape):
    """An incoming gradient as a contiguous tensor of ``shape`` (None stays None; an expanded zero becomes a real one)."""
    if g is None:
        return None
    return g.contiguous() if tuple(g.shape) == shape else g.expand(shape).contiguous()


class MvnSampleLogProb(torch.autograd.Function):
    """V1: ``(z [K, R, D], lp [K, R])``.  ``pathwise`` False (a non-reparameterised node): the draw is a constant and ``lp``
    keeps only its direct dependence on ``mean`` and ``tril``.  The backward reads the injected ``eps`` again, or regenerates
    the draw's noise from the saved ``(seed, call, rng_state)``: nothing of size ``[K, R, D]`` is kept for it."""

    @staticmethod
    def forward(ctx, mean, tril, eps, seed, call, rng_state, K, pathwise):
        z, lp = _mvn_hip.sample_logprob(mean, tril, K, eps=eps, seed=seed, call=call, rng_state=rng_state)
        ctx.set_materialize_grads(False)          # an output that did not enter the loss brings None, not zeros
        ctx.K, ctx.pathwise, ctx.seed, ctx.call = K, pathwise, seed, call
        ctx.save_for_backward(tril, eps, rng_state)
        ctx.shapes = (tuple(z.shape), tuple(lp.shape))
        if not pathwise:
            ctx.mark_non_differentiable(z)
        return z, lp

    @staticmethod
    @once_differentiable
    def backward(ctx, gz, glp):
        tril, eps, rng_state = ctx.saved_tensors
        none = (None,) * 6
        wm, wt = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not ctx.pathwise:
            gz = None
        if not (wm or wt) or (gz is None and glp is None):
            return (None, None) + none
        gz, glp = _dense(gz, ctx.shapes[0]), _dense(glp, ctx.shapes[1])
        gmean, gtril = _mvn_hip.sample_logprob_bwd(tril, ctx.K, ctx.pathwise, eps=eps, seed=ctx.seed, call=ctx.call,
                                                   rng_state=rng_state, gz=gz, glp=glp, want_gmean=wm, want_gtril=wt)
        return (gmean, gtril) + none


class MvnLogProb(torch.autograd.Function):
    """V2: ``lp [K, R]`` of a given ``x`` (``[K, R, D]``, or ``[1, R, D]`` for a value shared by the particles)."""

    @staticmethod
    def forward(ctx, mean, tril, x, K):
        ctx.set_materialize_grads(False)          # an output that did not enter the loss brings None, not zeros
        ctx.K = K
        ctx.save_for_backward(mean, tril, x)
        return _mvn_hip.logprob(mean, tril, K, x)

    @staticmethod
    @once_differentiable
    def backward(ctx, glp):
        mean, tril, x = ctx.saved_tensors
        wm, wt, wx = ctx.needs_input_grad[:3]
        if glp is None or not (wm or wt or wx):
            return None, None, None, None
        gx, gmean, gtril = _mvn_hip.logprob_bwd(mean, tril, ctx.K, x, glp.contiguous(), want_gx=wx, want_gmean=wm, want_gtril=wt)
        if wx:
            gx = gx.sum(0, keepdim=True) if x.shape[0] != gx.shape[0] else gx
            gx = gx.reshape(x.shape)
        return gmean, gtril, gx, None
