"""The autograd Function of GPConditional over the kernels of include/zs_gp.h (``zhusuan._gp_hip``, imported at call time:
``import zhusuan`` loads neither that module nor its library), and the torch composition of the same formula for everything outside
their domain.  ``x`` is ``[N, d]``, ``inducing`` ``[M, d]``, ``lengthscale`` ``[d]``, ``amplitude`` ``[1]``, ``kzz_tril``
``[M, M]``, ``fz`` ``[K, M]``."""
import torch
from torch.autograd.function import once_differentiable

# zs_gp_max_inducing() per element size / zs_gp_max_input_dim(), restated so that routing does not import the binding; checked when
# the library loads
MAX_INDUCING = {4: 128, 8: 64}
MAX_INPUT_DIM = 64
MAX_PARTICLES = 65536


class GPMoments(torch.autograd.Function):
    """``(mean [K, N], var [N])``.  The forward keeps its operands and the small ``prep`` workspace (M (M + 2 K) elements); the
    backward recomputes the strips of K_xz: nothing of size ``[N, M]`` is saved."""

    @staticmethod
    def forward(ctx, x, inducing, lengthscale, amplitude, kzz_tril, fz):
        from .. import _gp_hip
        prep = _gp_hip.prepare(kzz_tril, fz)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(x, inducing, lengthscale, amplitude, prep)
        ctx.K = fz.shape[0]
        return _gp_hip.moments(x, inducing, lengthscale, amplitude, prep, ctx.K)

    @staticmethod
    @once_differentiable
    def backward(ctx, gmean, gvar):
        from .. import _gp_hip
        x, inducing, lengthscale, amplitude, prep = ctx.saved_tensors
        need = ctx.needs_input_grad
        if (gmean is None and gvar is None) or not any(need):
            return (None,) * 6
        grads = _gp_hip.moments_bwd(x, inducing, lengthscale, amplitude, prep, None if gmean is None else gmean.contiguous(),
                                    None if gvar is None else gvar.contiguous(), ctx.K, want_gx=need[0])
        return tuple(g if w else None for g, w in zip(grads, need))


def torch_moments(x, inducing, lengthscale, amplitude, kzz_tril, fz):
    """The torch composition, in the form of the kernels (include/zs_gp.h): the square expanded around the mean of the scaled
    inducing inputs, two triangular solves.  Only the lower triangle of ``kzz_tril`` is read.  It materialises ``K_xz [N, M]``."""
    zs = inducing / lengthscale
    cen = zs.mean(0)
    zs, xs = zs - cen, x / lengthscale - cen
    score = xs @ zs.t() - 0.5 * ((xs * xs).sum(-1)[:, None] + (zs * zs).sum(-1)[None, :])
    amp2 = amplitude.reshape(()) ** 2
    kxz = amp2 * torch.exp(score)
    tril = torch.tril(kzz_tril)
    a = torch.linalg.solve_triangular(tril, kxz.t(), upper=False)          # [M, N]
    w = torch.linalg.solve_triangular(tril, fz.t(), upper=False)           # [M, K]
    return w.t() @ a, amp2 - (a * a).sum(0)
