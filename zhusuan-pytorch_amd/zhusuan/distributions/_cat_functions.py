"""Autograd Functions of the categorical families over the kernels of include/zs_cat.h (``zhusuan._cat_hip``, looked up at call
time).  ``logits`` is always the contiguous ``[R, N]`` view, per-particle operands are ``[K, R(, N)]``; one launch forward, one
launch backward.  The temperature of the relaxed families is a Python float here and has no gradient."""
import torch
from torch.autograd.function import once_differentiable

from .. import _cat_hip


def _dense(g, like):
    """An incoming gradient as a contiguous tensor (None stays None; an expanded zero becomes a real one)."""
    if g is None:
        return None
    return g.contiguous() if g.shape == like.shape else g.expand(like.shape).contiguous()


class CatSampleLogProb(torch.autograd.Function):
    """C1: ``(idx [K, R] int64, onehot [K, R, N] or None, lp [K, R])``.  The draw has no gradient; ``lp`` has the score-function
    gradient w.r.t. ``logits`` (backward of C2 on the saved indices)."""

    @staticmethod
    def forward(ctx, logits, u, seed, call, rng_state, K, want_onehot):
        idx, onehot, lp = _cat_hip.sample_logprob(logits, K, u=u, seed=seed, call=call, rng_state=rng_state, want_index=True,
                                                  want_onehot=want_onehot)
        ctx.set_materialize_grads(False)          # an output that did not enter the loss brings None, not zeros
        ctx.K = K
        ctx.save_for_backward(logits, idx)
        ctx.mark_non_differentiable(idx)
        if onehot is not None:
            ctx.mark_non_differentiable(onehot)
        return idx, onehot, lp

    @staticmethod
    @once_differentiable
    def backward(ctx, gidx, gonehot, glp):
        logits, idx = ctx.saved_tensors
        glogits = None
        if ctx.needs_input_grad[0] and glp is not None:
            glogits, _ = _cat_hip.logprob_bwd(logits, ctx.K, _dense(glp, idx), idx=idx)
        return glogits, None, None, None, None, None, None


class CatLogProb(torch.autograd.Function):
    """C2: ``lp [K, R]`` of indices (``onehot_form`` False: int64 ``[K, R]``) or of weights (``[K, R, N]``)."""

    @staticmethod
    def forward(ctx, logits, value, K, onehot_form):
        ctx.set_materialize_grads(False)          # an output that did not enter the loss brings None, not zeros
        ctx.K, ctx.onehot_form = K, onehot_form
        ctx.save_for_backward(logits, value)
        if onehot_form:
            return _cat_hip.logprob(logits, K, x=value)
        return _cat_hip.logprob(logits, K, idx=value)

    @staticmethod
    @once_differentiable
    def backward(ctx, glp):
        logits, value = ctx.saved_tensors
        want_gx = ctx.onehot_form and ctx.needs_input_grad[1]
        if glp is None or not (ctx.needs_input_grad[0] or want_gx):
            return None, None, None, None
        g = glp.contiguous()
        if ctx.onehot_form:
            glogits, gx = _cat_hip.logprob_bwd(logits, ctx.K, g, x=value, want_gx=want_gx)
            return glogits, (gx.reshape(value.shape) if want_gx else None), None, None
        glogits, _ = _cat_hip.logprob_bwd(logits, ctx.K, g, idx=value)
        return glogits, None, None, None


class RelaxedSampleLogProb(torch.autograd.Function):
    """C3: ``(y [K, R, N], exp(y) or None, lp [K, R])``.  ``pathwise`` False (a non-reparameterised node): the draw is a
    constant and ``lp`` keeps only its direct dependence on ``logits`` (backward of C4 at the saved y)."""

    @staticmethod
    def forward(ctx, logits, u, seed, call, rng_state, K, tau, exp_space, pathwise):
        y, ey, lp = _cat_hip.relaxed_sample_logprob(logits, K, tau, exp_space, u=u, seed=seed, call=call, rng_state=rng_state)
        ctx.set_materialize_grads(False)          # an output that did not enter the loss brings None, not zeros
        ctx.K, ctx.tau, ctx.exp_space, ctx.pathwise = K, tau, exp_space, pathwise
        ctx.save_for_backward(logits, y)
        if not pathwise:
            ctx.mark_non_differentiable(y)
            if ey is not None:
                ctx.mark_non_differentiable(ey)
        return y, ey, lp

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, gey, glp):
        logits, y = ctx.saved_tensors
        none = (None,) * 8
        if not ctx.needs_input_grad[0]:
            return (None,) + none
        glp = None if glp is None else glp.contiguous()
        if not ctx.pathwise:
            if glp is None:
                return (None,) + none
            _, glogits = _cat_hip.relaxed_logprob_bwd(logits, ctx.K, ctx.tau, ctx.exp_space, y, glp, want_gy=False)
            return (glogits,) + none
        gy = _dense(gy, y)
        gey = _dense(gey, y) if ctx.exp_space else None
        if gy is None and gey is None and glp is None:
            return (None,) + none
        return (_cat_hip.relaxed_sample_logprob_bwd(logits, ctx.K, ctx.tau, ctx.exp_space, y, gy=gy, gey=gey, glp=glp),) + none


class RelaxedLogProb(torch.autograd.Function):
    """C4: ``lp [K, R]`` of a given ``y [K, R, N]`` (``exp_space``: the Concrete density of ``exp(y)``)."""

    @staticmethod
    def forward(ctx, logits, y, K, tau, exp_space):
        ctx.set_materialize_grads(False)          # an output that did not enter the loss brings None, not zeros
        ctx.K, ctx.tau, ctx.exp_space = K, tau, exp_space
        ctx.save_for_backward(logits, y)
        return _cat_hip.relaxed_logprob(logits, K, tau, exp_space, y)

    @staticmethod
    @once_differentiable
    def backward(ctx, glp):
        logits, y = ctx.saved_tensors
        wl, wy = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if glp is None or not (wl or wy):
            return None, None, None, None, None
        gy, glogits = _cat_hip.relaxed_logprob_bwd(logits, ctx.K, ctx.tau, ctx.exp_space, y, glp.contiguous(), want_gy=wy,
                                                   want_glogits=wl)
        return glogits, (gy.reshape(y.shape) if wy else None), None, None, None
