"""Autograd Functions of MatrixVariateNormalCholesky over the kernels of include/zs_matvar.h (``zhusuan._matvar_hip``, imported at
call time: ``import zhusuan`` loads neither that module nor its library), and the torch composition that wider events and CPU
tensors run.  ``mean`` is always the contiguous ``[R, n, p]`` view, ``u`` the ``[R, n, n]`` and ``v`` the ``[R, p, p]`` one,
per-particle operands are ``[K, R(, n, p)]``."""
import math

import torch
from torch.autograd.function import once_differentiable

MAX_DIM = {4: 128, 8: 64}          # zs_matvar_max_dim by element size, restated so that routing does not import the binding; checked when the library loads
GRID_TARGET, MAX_SHARES = 256, 16          # of zs_matvar_shares, likewise


def shares(K, R):
    """``zs_matvar_shares(K, R)`` restated (checked against the library when it loads): the contiguous shares the backward
    kernels cut a row's K particles into, one workgroup each."""
    if K < 1 or R < 1:
        return 0
    s = min(-(-GRID_TARGET // R), MAX_SHARES, K)
    per = -(-K // s)
    return -(-K // per)


def _dense(g, shape):
    """An incoming gradient as a contiguous tensor of ``shape`` (None stays None; an expanded zero becomes a real one)."""
    if g is None:
        return None
    return g.contiguous() if tuple(g.shape) == shape else g.expand(shape).contiguous()


class MatvarSampleLogProb(torch.autograd.Function):
    """M1: ``(z [K, R, n, p], lp [K, R])``, one launch.  ``pathwise``: the backward is M1's, from the injected ``eps`` or from
    the noise regenerated with the saved ``(seed, call, rng_state)`` -- nothing of size ``[K, R, n, p]`` is kept for it.
    Otherwise (a non-reparameterised node) the draw is a constant, and ``lp`` is differentiated through M2's backward at that
    value, which is all that is kept."""

    @staticmethod
    def forward(ctx, mean, u, v, eps, seed, call, rng_state, K, pathwise):
        from .. import _matvar_hip
        z, lp = _matvar_hip.sample_logprob(mean, u, v, K, eps=eps, seed=seed, call=call, rng_state=rng_state)
        ctx.set_materialize_grads(False)          # an output that did not enter the loss brings None, not zeros
        ctx.K, ctx.pathwise, ctx.seed, ctx.call = K, pathwise, seed, call
        ctx.shapes = (tuple(z.shape), tuple(lp.shape))
        if pathwise:
            ctx.save_for_backward(mean, u, v, eps, rng_state)
        else:
            ctx.save_for_backward(mean, u, v, z)
            ctx.mark_non_differentiable(z)
        return z, lp

    @staticmethod
    @once_differentiable
    def backward(ctx, gz, glp):
        from .. import _matvar_hip
        want = tuple(ctx.needs_input_grad[:3])
        none = (None,) * 6
        glp = _dense(glp, ctx.shapes[1])
        if ctx.pathwise:
            mean, u, v, eps, rng_state = ctx.saved_tensors
            gz = _dense(gz, ctx.shapes[0])
            if not any(want) or (gz is None and glp is None):
                return (None, None, None) + none
            grads = _matvar_hip.sample_logprob_bwd(mean, u, v, ctx.K, eps=eps, seed=ctx.seed, call=ctx.call, rng_state=rng_state,
                                                   gz=gz, glp=glp, want=want)
        else:
            mean, u, v, z = ctx.saved_tensors
            if not any(want) or glp is None:
                return (None, None, None) + none
            grads = _matvar_hip.logprob_bwd(mean, u, v, ctx.K, z, glp, want_gx=False, want=want)[1:]
        return tuple(grads) + none


class MatvarLogProb(torch.autograd.Function):
    """M2: ``lp [K, R]`` of a given ``x [K, R, n, p]``, one launch; the backward launches once for ``gx`` alone and twice when a
    parameter needs its gradient.  (The parameters carry no particle axis, so a value never arrives without one where K > 1:
    the shared-value period of the ABI is not used from here.)"""

    @staticmethod
    def forward(ctx, mean, u, v, x, K):
        from .. import _matvar_hip
        ctx.set_materialize_grads(False)
        ctx.K = K
        ctx.save_for_backward(mean, u, v, x)
        return _matvar_hip.logprob(mean, u, v, K, x)

    @staticmethod
    @once_differentiable
    def backward(ctx, glp):
        from .. import _matvar_hip
        mean, u, v, x = ctx.saved_tensors
        want, wx = tuple(ctx.needs_input_grad[:3]), ctx.needs_input_grad[3]
        if glp is None or not (any(want) or wx):
            return None, None, None, None, None
        gx, gmean, gu, gv = _matvar_hip.logprob_bwd(mean, u, v, ctx.K, x, glp.contiguous(), want_gx=wx, want=want)
        return gmean, gu, gv, gx, None


def _log_norm(U, V):
    n, p = U.shape[-1], V.shape[-1]
    return (-0.5 * n * p * math.log(2.0 * math.pi) - p * torch.log(torch.diagonal(U, dim1=-2, dim2=-1)).sum(-1)
            - n * torch.log(torch.diagonal(V, dim1=-2, dim2=-1)).sum(-1))


def torch_sample(mean, u, v, eps):
    """The torch composition of the draw and of its density: ``(mean + U eps V^T, c - 1/2 |eps|^2)``."""
    U, V = torch.tril(u), torch.tril(v)
    z = mean + U @ eps @ V.transpose(-1, -2)
    return z, _log_norm(U, V) - 0.5 * (eps * eps).sum((-1, -2))


def torch_log_prob(mean, u, v, x):
    """The torch composition of the density: two ``solve_triangular``."""
    U, V = torch.tril(u), torch.tril(v)
    d = x - mean
    n, p = d.shape[-2:]
    lead = d.shape[:-2]
    y = torch.linalg.solve_triangular(U.expand(lead + (n, n)), d, upper=False)                              # U^-1 D
    a = torch.linalg.solve_triangular(V.expand(lead + (p, p)), y.transpose(-1, -2), upper=False)            # (U^-1 D V^-T)^T
    return _log_norm(U, V) - 0.5 * (a * a).sum((-1, -2))
