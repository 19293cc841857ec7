"""MultivariateNormalLowRank: a normal over D-vectors with covariance ``diag(cov_diag) + cov_factor cov_factor^T``
(``torch.distributions.LowRankMultivariateNormal``'s parameterisation; SWAG-style posteriors) -- the correlated Gaussian for a
wide flat latent: a variational posterior over a BNN's whole weight vector, a VAE latent a few hundred wide.  It has
``D (r + 2)`` parameters and never forms a D x D matrix.  On a HIP device, for ranks up to 64 and D up to 65 536, the draw, the
log-density of a value and their gradients come from the fused matrix-core kernels of include/zs_lowrank.h; CPU tensors, higher
ranks and wider events run the torch composition of the same Woodbury form; ``last_path`` / ``zhusuan.explain`` say which
(DESIGN.md 4p)."""
import torch

from .base import Distribution
from .categorical import _numel, sum_trailing
from .utils import assert_same_log_float_dtype
from . import _lowrank_functions as _F
from .. import _hip, _ops, _rng
from .._shapes import broadcast_shapes
from ..utils import note_path

__all__ = ['MultivariateNormalLowRank']

SAMPLE_KERNEL = "zs_lowrank_sample: mean + sqrt(d) eps_D + eps_r W^T, the rank product on the matrix cores"
LOGPROB_KERNELS = ("zs_lowrank_prepare + zs_lowrank_logprob: the capacitance and u = y Wd as matrix-core products over streamed "
                   "panels of the factor; zs_lowrank_logprob_bwd backward")
COMPOSITION = "torch composition (Woodbury form: Cholesky of the r x r capacitance)"


class MultivariateNormalLowRank(Distribution):
    """
    :param mean: float tensor ``[..., D]``.
    :param cov_factor: float tensor ``[..., D, r]``, the low-rank factor ``W`` of the covariance.
    :param cov_diag: float tensor ``[..., D]``, its diagonal part; must be positive, which is not checked.
    :param is_reparameterized: False detaches the draw (its log-density keeps the direct dependence on the parameters).
    ``batch_shape`` is the broadcast of the three batch shapes; samples are ``[K] + batch_shape + [D]``.  The density of the
    node's own draw is the density kernel at that draw: autograd composes the two.
    """
    _event_ndims = 1
    _nonreparam_draw_has_zero_grad = True

    def __init__(self, mean, cov_factor, cov_diag, dtype=None, is_reparameterized=True, use_path_derivative=False, group_ndims=0,
                 device=None, **kwargs):
        device = _hip.resolve_device(device, mean, cov_factor, cov_diag)
        self._mean = torch.as_tensor(mean, dtype=dtype).to(device)
        self._cov_factor = torch.as_tensor(cov_factor, dtype=dtype).to(device)
        self._cov_diag = torch.as_tensor(cov_diag, dtype=dtype).to(device)
        dtype = assert_same_log_float_dtype([(self._mean, 'MultivariateNormalLowRank.mean'),
                                             (self._cov_factor, 'MultivariateNormalLowRank.cov_factor'),
                                             (self._cov_diag, 'MultivariateNormalLowRank.cov_diag')])
        if self._mean.dim() < 1 or self._mean.shape[-1] < 1:
            raise ValueError("mean must have a last axis of at least one dimension")
        D = int(self._mean.shape[-1])
        if self._cov_factor.dim() < 2 or self._cov_factor.shape[-2] != D or self._cov_factor.shape[-1] < 1:
            raise ValueError("cov_factor must have shape [..., %d, r] with r >= 1 (the last axis of mean has %d entries), got %s"
                             % (D, D, tuple(self._cov_factor.shape)))
        if self._cov_diag.dim() < 1 or self._cov_diag.shape[-1] != D:
            raise ValueError("cov_diag must have shape [..., %d], got %s" % (D, tuple(self._cov_diag.shape)))
        try:
            self._batch = torch.Size(broadcast_shapes(tuple(self._mean.shape[:-1]), tuple(self._cov_factor.shape[:-2]),
                                                      tuple(self._cov_diag.shape[:-1])))
        except RuntimeError as e:
            raise ValueError("the batch shapes of mean %s, cov_factor %s and cov_diag %s do not broadcast: %s"
                             % (tuple(self._mean.shape[:-1]), tuple(self._cov_factor.shape[:-2]), tuple(self._cov_diag.shape[:-1]), e))
        if use_path_derivative:
            raise NotImplementedError("MultivariateNormalLowRank: use_path_derivative is not implemented")
        self._n_dims, self._rank = D, int(self._cov_factor.shape[-1])
        super(MultivariateNormalLowRank, self).__init__(dtype=dtype, is_continuous=True, is_reparameterized=is_reparameterized,
                                                        use_path_derivative=use_path_derivative, group_ndims=group_ndims,
                                                        device=device, **kwargs)
        self.last_path = None          # which path the last sample / log_prob ran on (zhusuan.explain)

    @property
    def mean(self):
        return self._mean

    @property
    def cov_factor(self):
        return self._cov_factor

    @property
    def cov_diag(self):
        return self._cov_diag

    @property
    def n_dims(self):
        return self._n_dims

    @property
    def rank(self):
        return self._rank

    def _batch_shape(self):
        return self._batch

    def _outside(self):
        """Why the kernels do not take this distribution, or None."""
        if self._mean.device.type != "cuda":
            return "the operands are on the CPU"
        if self._rank > _F.MAX_RANK:
            return "ranks above %d are outside the fused kernels' domain (zs_lowrank_max_rank)" % _F.MAX_RANK
        if self._n_dims > _F.MAX_DIM:
            return "events wider than %d are outside the fused kernels' domain (zs_lowrank_max_dim)" % _F.MAX_DIM
        return None

    def _flat_params(self, batch):
        """(mean [R, D], factor [R, D, r], diag [R, D]) expanded to ``batch`` and contiguous; autograd sums the expanded gradient."""
        D, r, batch = self._n_dims, self._rank, tuple(batch)
        return (self._mean.expand(batch + (D,)).reshape(-1, D).contiguous(),
                self._cov_factor.expand(batch + (D, r)).reshape(-1, D, r).contiguous(),
                self._cov_diag.expand(batch + (D,)).reshape(-1, D).contiguous())

    def _sample(self, n_samples=1, **kwargs):
        K = int(n_samples)
        lead = (K,) if K > 1 else ()
        batch, D, r = tuple(self._batch), self._n_dims, self._rank
        shape = lead + batch + (D + r,)
        why = self._outside()
        if why is None and _numel(batch) == 0:
            why = "there are no rows"
        eps = _rng.pop_injected(shape, self._mean.device, self._dtype, kind="normal")
        if why is not None:
            if eps is None:
                if self._mean.device.type == "cuda":
                    seed, call, rng_state = _rng.next_call(self._mean.device)
                    eps = _ops.philox_normal(shape, self._mean.device, seed, call, rng_state, self._dtype)
                else:
                    eps = torch.randn(shape, dtype=self._dtype)
            z = _F.torch_sample(self._mean, self._cov_factor, self._cov_diag, eps)
            note_path(self, "torch composition (mean + sqrt(d) eps_D + W eps_r)", why)
        else:
            seed, call, rng_state = (0, 0, None) if eps is not None else _rng.next_call(self._mean.device)
            mean, factor, diag = self._flat_params(batch)
            z = _F.LowRankSample.apply(mean, factor, diag, eps, seed, call, rng_state, K).reshape(lead + batch + (D,))
            note_path(self, SAMPLE_KERNEL)
        if not self._is_reparameterized:
            z = z.detach()
        self.sample_cache = z
        return z

    def _log_prob_sum(self, given=None, n_fold=0):
        x = self.sample_cache if given is None else given
        if x is None:
            raise RuntimeError("MultivariateNormalLowRank.log_prob(None) needs a cached sample: call sample() first")
        x = torch.as_tensor(x, dtype=self._dtype).to(self._mean.device)
        D = self._n_dims
        if x.dim() < 1 or x.shape[-1] != D:
            raise ValueError("the last axis of the value must have %d entries, got shape %s" % (D, tuple(x.shape)))
        batch = tuple(self._batch)
        full = tuple(broadcast_shapes(tuple(x.shape[:-1]), batch))
        why = self._outside()
        if why is None and _numel(full) == 0:
            why = "there are no rows"
        if why is not None:
            lp = _F.torch_log_prob(self._mean, self._cov_factor, self._cov_diag, x).expand(full)
            note_path(self, COMPOSITION, why)
            return sum_trailing(lp, n_fold)
        lead, tail = full[:len(full) - len(batch)], full[len(full) - len(batch):]
        K, R = _numel(lead), _numel(tail)
        if tuple(x.shape[:-1]) == tail:          # no particle axis: the kernels share the value among the particles
            rows = x.reshape(1, R, D).contiguous()
        else:
            rows = x.expand(full + (D,)).reshape(K, R, D).contiguous()
        mean, factor, diag = self._flat_params(tail)
        lp = _F.LowRankLogProb.apply(mean, factor, diag, rows, K)
        note_path(self, LOGPROB_KERNELS)
        return sum_trailing(lp.reshape(full), n_fold)
