"""The autograd Function of NormalMixture over the kernels of include/zs_mix.h (``zhusuan._mix_hip``, imported at call time:
``import zhusuan`` loads neither that module nor its library), and the torch composition of everything outside their domain.
``logits`` is ``[C]``, ``mean`` and ``logstd`` are ``[C, D]``, ``x`` is the contiguous ``[R, D]`` view of the value."""
import math

import torch
from torch.autograd.function import once_differentiable

# zs_mix_max_dim() / zs_mix_max_components(), restated so that routing does not import the binding; checked when the library loads
MAX_DIM = 64
MAX_COMPONENTS = 65536


class MixtureLogProb(torch.autograd.Function):
    """``lp [R]``.  The forward keeps ``lp`` and the small ``prep`` workspace instead of anything of size ``[R, C]``; the backward
    recomputes the scores and launches ``zs_mix_grad_x`` only if ``x`` needs a gradient and ``zs_mix_grad_params`` only if a
    parameter does.  ``record`` (a dict of the caller's, may be None) receives ``needs_input_grad``, whether the ``dx`` launch
    ran and the number of elements of the partial workspace of the parameter gradients (None if they did not run)."""

    @staticmethod
    def forward(ctx, logits, mean, logstd, x, record):
        from .. import _mix_hip
        lp, prep = _mix_hip.logprob(logits, mean, logstd, x)
        ctx.save_for_backward(logits, mean, logstd, x, lp, prep)
        ctx.record = record
        ctx.set_materialize_grads(False)
        return lp

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from .. import _mix_hip
        logits, mean, logstd, x, lp, prep = ctx.saved_tensors
        needs = tuple(bool(n) for n in ctx.needs_input_grad[:4])
        dlogits = dmean = dlogstd = dx = part = None
        if g is not None:
            g = g.contiguous()
            if needs[3]:
                dx = _mix_hip.grad_x(mean, x, g, lp, prep)
            if any(needs[:3]):
                dlogits, dmean, dlogstd, part = _mix_hip.grad_params(logits, mean, logstd, x, g, lp, prep)
        if ctx.record is not None:
            ctx.record.update(needs_input_grad=needs, grad_x_ran=dx is not None,
                              grad_params_workspace_elems=None if part is None else part.numel())
        return (dlogits if needs[0] else None, dmean if needs[1] else None, dlogstd if needs[2] else None, dx, None)


def torch_log_prob(logits, mean, logstd, x):
    """The torch composition, in the matmul form of the kernels (include/zs_mix.h): the square is expanded around the
    per-dimension centre of the means, so the largest temporary is the ``[rows, C]`` score matrix, never ``[rows, C, D]``.  The
    centre cancels and carries no gradient.  ``x`` is ``[..., D]``."""
    D = mean.shape[-1]
    w = torch.exp(-2.0 * logstd)
    centre = mean.mean(0).detach()
    y, nu = x - centre, mean - centre
    b = torch.log_softmax(logits, -1) - logstd.sum(-1) - 0.5 * D * math.log(2.0 * math.pi) - 0.5 * (w * nu * nu).sum(-1)
    s = b + torch.cat([y, y * y], -1) @ torch.cat([w * nu, -0.5 * w], -1).t()
    return torch.logsumexp(s, -1)
