"""The autograd Functions of MultivariateNormalLowRank over the kernels of include/zs_lowrank.h (``zhusuan._lowrank_hip``,
imported at call time: ``import zhusuan`` loads neither that module nor its library), and the torch composition of everything
outside their domain.  ``mean`` and ``diag`` are the contiguous ``[R, D]`` views, ``factor`` the ``[R, D, r]`` one, per-particle
operands are ``[K, R(, D)]``."""
import math

import torch
from torch.autograd.function import once_differentiable

# zs_lowrank_max_dim() / zs_lowrank_max_rank(), restated so that routing does not import the binding; checked when the library loads
MAX_DIM = 65536
MAX_RANK = 64


class LowRankLogProb(torch.autograd.Function):
    """``lp [K, R]`` of a given ``x`` (``[K, R, D]``, or ``[1, R, D]`` for a value shared by the particles).  The forward keeps
    the small ``prep`` workspace; the backward recomputes ``u`` and writes the four gradients in two launches."""

    @staticmethod
    def forward(ctx, mean, factor, diag, x, K):
        from .. import _lowrank_hip
        prep = _lowrank_hip.prepare(factor, diag)
        ctx.set_materialize_grads(False)
        ctx.K = K
        ctx.save_for_backward(mean, factor, diag, x, prep)
        return _lowrank_hip.logprob(mean, factor, diag, prep, x, K)

    @staticmethod
    @once_differentiable
    def backward(ctx, glp):
        from .. import _lowrank_hip
        mean, factor, diag, x, prep = ctx.saved_tensors
        wm, wf, wd, wx = ctx.needs_input_grad[:4]
        if glp is None or not (wm or wf or wd or wx):
            return None, None, None, None, None
        gx, gmean, gfactor, gdiag = _lowrank_hip.logprob_bwd(mean, factor, diag, prep, x, glp.contiguous(), ctx.K, want_gx=wx)
        if wx:
            gx = gx.sum(0, keepdim=True) if x.shape[0] != gx.shape[0] else gx
            gx = gx.reshape(x.shape)
        return (gmean if wm else None, gfactor if wf else None, gdiag if wd else None, gx, None)


class LowRankSample(torch.autograd.Function):
    """``z [K, R, D]``.  The backward reads the injected ``eps [K, R, D + r]`` again, or regenerates the draw's noise from the
    saved ``(seed, call, rng_state)``: nothing of size ``[K, R, D]`` is kept for it."""

    @staticmethod
    def forward(ctx, mean, factor, diag, eps, seed, call, rng_state, K):
        from .. import _lowrank_hip
        ctx.set_materialize_grads(False)
        ctx.K, ctx.seed, ctx.call = K, seed, call
        ctx.save_for_backward(factor, diag, eps, rng_state)
        return _lowrank_hip.sample(mean, factor, diag, K, eps=eps, seed=seed, call=call, rng_state=rng_state)

    @staticmethod
    @once_differentiable
    def backward(ctx, gz):
        from .. import _lowrank_hip
        factor, diag, eps, rng_state = ctx.saved_tensors
        wm, wf, wd = ctx.needs_input_grad[:3]
        if gz is None or not (wm or wf or wd):
            return (None,) * 8
        gmean, gfactor, gdiag = _lowrank_hip.sample_bwd(factor, diag, gz.contiguous(), ctx.K, eps=eps, seed=ctx.seed, call=ctx.call,
                                                        rng_state=rng_state)
        return (gmean if wm else None, gfactor if wf else None, gdiag if wd else None) + (None,) * 5


def torch_log_prob(mean, factor, diag, x):
    """The torch composition, in the Woodbury form of the kernels (include/zs_lowrank.h): the capacitance ``I + W^T W / d`` is
    the only matrix that is factored.  ``mean``, ``diag`` are ``[..., D]``, ``factor`` ``[..., D, r]``, ``x`` broadcasts."""
    D, r = factor.shape[-2:]
    wd = factor / diag[..., None]
    cap = torch.eye(r, dtype=factor.dtype, device=factor.device) + factor.transpose(-1, -2) @ wd
    chol = torch.linalg.cholesky(cap)
    y = x - mean
    u = (y[..., None, :] @ wd)[..., 0, :]
    t = torch.linalg.solve_triangular(chol.expand(u.shape[:-1] + (r, r)), u[..., None], upper=False)[..., 0]
    maha = (y * y / diag).sum(-1) - (t * t).sum(-1)
    logdet = torch.log(diag).sum(-1) + 2.0 * torch.log(torch.diagonal(chol, dim1=-2, dim2=-1)).sum(-1)
    return -0.5 * maha - 0.5 * logdet - 0.5 * D * math.log(2.0 * math.pi)


def torch_sample(mean, factor, diag, eps):
    """``mean + sqrt(diag) eps_D + W eps_r`` from one noise tensor ``[..., D + r]`` (the kernels' layout)."""
    D = factor.shape[-2]
    return mean + torch.sqrt(diag) * eps[..., :D] + (factor @ eps[..., D:, None])[..., 0]
