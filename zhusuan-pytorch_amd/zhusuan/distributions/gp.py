"""GPConditional: the predictive distribution of a sparse variational Gaussian process at inputs ``x`` given function values at
inducing inputs (upstream ZhuSuan's ``gp_conditional(z, fz, x, full_cov=False, kernel, Kzz_chol)`` with an ARD squared-exponential
kernel) -- an independent normal per input with

    mean[k, n] = A_n^T L^-1 fz_k,   var[n] = a^2 - |A_n|^2,   A_n = L^-1 k(Z, x_n),   L L^T = k(Z, Z) + jitter I.

On a HIP device, for up to 128 (float32) / 64 (float64) inducing inputs and inputs up to 64 wide, the two moments and their
gradients come from the fused matrix-core kernels of include/zs_gp.h, which never store the cross-covariance ``[N, M]``; CPU
tensors and shapes outside that domain run the torch composition of the same formula; ``last_path`` / ``zhusuan.explain`` say
which.  Draws and densities are those of the package's ``Normal`` on the two moments."""
import torch

from .base import Distribution
from .categorical import _numel
from .normal import Normal
from .utils import assert_same_log_float_dtype
from . import _gp_functions as _F
from .. import _hip
from ..utils import note_path

__all__ = ['GPConditional']

KERNELS = ("zs_gp_prepare + zs_gp_moments: the strips of K_xz in matrix-core accumulators, A = K_xz L^-T and mean = K_xz c as "
           "products on them; zs_gp_moments_bwd backward")
COMPOSITION = "torch composition (K_xz materialised, two triangular solves)"


class GPConditional(Distribution):
    """
    :param x: float tensor ``[N, d]``, the inputs.
    :param inducing: float tensor ``[M, d]``, the inducing inputs.
    :param f_inducing: float tensor ``[..., M]``, the function values at the inducing inputs; its leading axes are the particles.
    :param kzz_tril: float tensor ``[M, M]``, the lower Cholesky factor of ``k(inducing, inducing) + jitter I``
        (``GPConditional.gram_tril``); only its lower triangle is read.
    :param lengthscale: float tensor ``[d]`` (or a scalar), positive, which is not checked.
    :param amplitude: float scalar, positive, which is not checked: ``k(p, p) = amplitude^2``.
    :param is_reparameterized: False detaches the draw.
    ``batch_shape`` is ``f_inducing.shape[:-1] + [N]``; ``mean`` has that shape, ``std`` is ``[N]``.
    """

    def __init__(self, x, inducing, f_inducing, kzz_tril, lengthscale, amplitude, group_ndims=0, is_reparameterized=True, dtype=None,
                 device=None, **kwargs):
        device = _hip.resolve_device(device, x, inducing, f_inducing, kzz_tril, lengthscale, amplitude)
        self._x, self._inducing, self._fz, self._tril, self._lengthscale, self._amplitude = (
            torch.as_tensor(t, dtype=dtype).to(device) for t in (x, inducing, f_inducing, kzz_tril, lengthscale, amplitude))
        dtype = assert_same_log_float_dtype([(self._x, 'GPConditional.x'), (self._inducing, 'GPConditional.inducing'),
                                             (self._fz, 'GPConditional.f_inducing'), (self._tril, 'GPConditional.kzz_tril'),
                                             (self._lengthscale, 'GPConditional.lengthscale'),
                                             (self._amplitude, 'GPConditional.amplitude')])
        if self._x.dim() != 2 or self._x.shape[1] < 1:
            raise ValueError("x must have shape [N, d] with d >= 1, got %s" % (tuple(self._x.shape),))
        N, d = (int(s) for s in self._x.shape)
        if self._inducing.dim() != 2 or self._inducing.shape[0] < 1 or self._inducing.shape[1] != d:
            raise ValueError("inducing must have shape [M, %d] with M >= 1 (x is %s), got %s"
                             % (d, tuple(self._x.shape), tuple(self._inducing.shape)))
        M = int(self._inducing.shape[0])
        if self._fz.dim() < 1 or self._fz.shape[-1] != M:
            raise ValueError("f_inducing must have shape [..., %d] (inducing has %d rows), got %s" % (M, M, tuple(self._fz.shape)))
        if tuple(self._tril.shape) != (M, M):
            raise ValueError("kzz_tril must have shape [%d, %d], got %s" % (M, M, tuple(self._tril.shape)))
        if self._lengthscale.dim() > 1 or (self._lengthscale.dim() == 1 and self._lengthscale.shape[0] not in (1, d)):
            raise ValueError("lengthscale must be a scalar or have shape [%d], got %s" % (d, tuple(self._lengthscale.shape)))
        if self._amplitude.numel() != 1:
            raise ValueError("amplitude must be a scalar, got shape %s" % (tuple(self._amplitude.shape),))
        self._n, self._m, self._d = N, M, d
        self._batch = torch.Size(tuple(self._fz.shape[:-1]) + (N,))
        super(GPConditional, self).__init__(dtype=dtype, is_continuous=True, is_reparameterized=is_reparameterized,
                                            group_ndims=group_ndims, device=device, **kwargs)
        self.last_path = None          # which path the moments ran on (zhusuan.explain)
        self._moments = None
        self._normal = None

    @staticmethod
    def gram_tril(inducing, lengthscale, amplitude, jitter=1e-6):
        """The lower Cholesky factor of ``k(inducing, inducing) + jitter I`` in torch ops (M is small; autograd composes)."""
        zs = inducing / lengthscale
        diff = zs[:, None, :] - zs[None, :, :]
        gram = amplitude ** 2 * torch.exp(-0.5 * (diff * diff).sum(-1))
        return torch.linalg.cholesky(gram + jitter * torch.eye(zs.shape[0], dtype=zs.dtype, device=zs.device))

    def _batch_shape(self):
        return self._batch

    def _outside(self):
        """Why the kernels do not take this distribution, or None."""
        cap = _F.MAX_INDUCING[self._x.element_size()]
        if self._x.device.type != "cuda":
            return "the operands are on the CPU"
        if self._m > cap:
            return "more than %d inducing inputs are outside the fused kernels' domain (zs_gp_max_inducing)" % cap
        if self._d > _F.MAX_INPUT_DIM:
            return "inputs wider than %d are outside the fused kernels' domain (zs_gp_max_input_dim)" % _F.MAX_INPUT_DIM
        if _numel(self._fz.shape[:-1]) > _F.MAX_PARTICLES:
            return "more than %d particles are outside the fused kernels' domain" % _F.MAX_PARTICLES
        if self._n == 0 or _numel(self._fz.shape[:-1]) == 0:
            return "there are no rows"
        return None

    def _mean_var(self):
        if self._moments is None:
            lead = tuple(self._fz.shape[:-1])
            fz = self._fz.reshape(-1, self._m)
            length = self._lengthscale.expand(self._d) if self._lengthscale.dim() == 1 else self._lengthscale.reshape(1).expand(self._d)
            amp = self._amplitude.reshape(1)
            why = self._outside()
            if why is not None:
                mean, var = _F.torch_moments(self._x, self._inducing, length, amp, self._tril, fz)
                note_path(self, COMPOSITION, why)
            else:
                mean, var = _F.GPMoments.apply(self._x.contiguous(), self._inducing.contiguous(), length.contiguous(), amp.contiguous(),
                                               self._tril.contiguous(), fz.contiguous())
                note_path(self, KERNELS)
            self._moments = (mean.reshape(lead + (self._n,)), var)
        return self._moments

    @property
    def mean(self):
        return self._mean_var()[0]

    @property
    def var(self):
        return self._mean_var()[1]

    @property
    def std(self):
        return torch.sqrt(torch.clamp(self._mean_var()[1], min=0))

    def _moment_normal(self):
        if self._normal is None:
            self._normal = Normal(self.mean, std=self.std, is_reparameterized=self._is_reparameterized, device=self._x.device)
        return self._normal

    def _sample(self, n_samples=1, **kwargs):
        self.sample_cache = self._moment_normal().sample(int(n_samples) if int(n_samples) > 1 else None, **kwargs)
        return self.sample_cache

    def _log_prob_sum(self, given=None, n_fold=0):
        x = self.sample_cache if given is None else given
        if x is None:
            raise RuntimeError("GPConditional.log_prob(None) needs a cached sample: call sample() first")
        return self._moment_normal()._log_prob_sum(x, n_fold)
