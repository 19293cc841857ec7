"""MultivariateNormalCholesky (upstream ZhuSuan's ``multivariate.MultivariateNormalCholesky``; the PyTorch reference dropped
it): a normal with mean ``mean`` and covariance ``L L^T``, ``L = cov_tril`` lower triangular.  Up to 64 dimensions the draw and
its log-density come from the fused HIP kernel V1, the density of a given value from V2 (include/zs_mvn.h): one launch each way.
Wider rows run the torch composition on the device; ``last_path`` / ``zhusuan.explain`` say which."""
import math

import torch

from .base import Distribution
from .categorical import _numel, sum_trailing
from .utils import assert_same_log_float_dtype
from . import _mvn_functions as _F
from .. import _hip, _mvn_hip, _ops, _rng
from .._shapes import broadcast_shapes
from ..utils import note_path

__all__ = ['MultivariateNormalCholesky']

WIDE = "rows wider than %d dimensions are outside the fused kernels' domain (zs_mvn_max_dim)" % _mvn_hip.MAX_DIM


def fold_particles(K, R, D):
    """Whether a given value of K particles over R rows goes to the kernels as K R rows of one particle (parameters expanded).
    The backward kernels give a lane group a ROW and walk its particles in turn (include/zs_mvn.h): with few rows and many
    particles -- one ``mean [D]`` against a batch of observations -- they would run on a wave or two.  Autograd sums the
    expanded parameters' gradient, so few rows with more than a handful of particles are folded."""
    lanes = 1
    while lanes < D:
        lanes *= 2
    return K > 8 and R * lanes < 4096


class MultivariateNormalCholesky(Distribution):
    """
    :param mean: float tensor ``[..., D]``.
    :param cov_tril: float tensor ``[..., D, D]``, the lower-triangular Cholesky factor ``L`` of the covariance.  Only its lower
        triangle is read (the gradient's upper triangle is zero); the diagonal must be positive, which is not checked: a zero or
        negative entry gives ``-inf`` / NaN log-densities.
    :param is_reparameterized: False detaches the draw (its log-density keeps the direct dependence on the parameters).
    ``batch_shape`` is the broadcast of ``mean.shape[:-1]`` and ``cov_tril.shape[:-2]``; samples are ``[K] + batch_shape + [D]``.
    """
    _event_ndims = 1
    _nonreparam_draw_has_zero_grad = True

    def __init__(self, mean, cov_tril, dtype=None, is_reparameterized=True, use_path_derivative=False, group_ndims=0,
                 device=None, **kwargs):
        device = _hip.resolve_device(device, mean, cov_tril)
        self._mean = torch.as_tensor(mean, dtype=dtype).to(device)
        self._cov_tril = torch.as_tensor(cov_tril, dtype=dtype).to(device)
        dtype = assert_same_log_float_dtype([(self._mean, 'MultivariateNormalCholesky.mean'),
                                             (self._cov_tril, 'MultivariateNormalCholesky.cov_tril')])
        if self._mean.dim() < 1 or self._mean.shape[-1] < 1:
            raise ValueError("mean must have a last axis of at least one dimension")
        D = int(self._mean.shape[-1])
        if self._cov_tril.dim() < 2 or tuple(self._cov_tril.shape[-2:]) != (D, D):
            raise ValueError("cov_tril must have shape [..., %d, %d] (the last axis of mean has %d entries), got %s"
                             % (D, D, D, tuple(self._cov_tril.shape)))
        try:
            self._batch = torch.Size(broadcast_shapes(tuple(self._mean.shape[:-1]), tuple(self._cov_tril.shape[:-2])))
        except RuntimeError as e:
            raise ValueError("the batch shapes of mean %s and cov_tril %s do not broadcast: %s"
                             % (tuple(self._mean.shape[:-1]), tuple(self._cov_tril.shape[:-2]), e))
        if use_path_derivative:
            raise NotImplementedError("MultivariateNormalCholesky: use_path_derivative is not implemented (the density of the "
                                      "node's own draw comes out of the sampling kernel together with the draw)")
        self._n_dims = D
        super(MultivariateNormalCholesky, self).__init__(dtype=dtype, is_continuous=True, is_reparameterized=is_reparameterized,
                                                         use_path_derivative=use_path_derivative, group_ndims=group_ndims,
                                                         device=device, **kwargs)
        self._fused = None          # (sample tensor, its log-density over the batch shape, 0)
        self.last_path = None          # which kernel the last sample / log_prob ran on (zhusuan.explain)

    @property
    def mean(self):
        return self._mean

    @property
    def cov_tril(self):
        return self._cov_tril

    @property
    def n_dims(self):
        return self._n_dims

    def _batch_shape(self):
        return self._batch

    def _flat_params(self, batch):
        """(mean [R, D], tril [R, D, D]) expanded to ``batch`` and contiguous; autograd sums the expanded gradient."""
        D = self._n_dims
        batch = tuple(batch)
        mean = self._mean.expand(batch + (D,)).reshape(-1, D).contiguous()
        tril = self._cov_tril.expand(batch + (D, D)).reshape(-1, D, D).contiguous()
        return mean, tril

    def _noise(self, shape):
        """(eps, seed, call, rng_state) of one draw: the injected / reference-stream normals, else the next Philox call."""
        eps = _rng.pop_injected(shape, self._mean.device, self._dtype, kind="normal")
        if eps is not None:
            return eps.contiguous(), 0, 0, None
        seed, call, rng_state = _rng.next_call(self._mean.device)
        return None, seed, call, rng_state

    @staticmethod
    def _torch_log_prob(mean, tril, x):
        """The torch composition of the density (rows wider than the kernels take)."""
        D = mean.shape[-1]
        L = torch.tril(tril)
        diff = (x - mean)[..., None]
        y = torch.linalg.solve_triangular(L.expand(diff.shape[:-2] + (D, D)), diff, upper=False)[..., 0]
        return (-0.5 * D * math.log(2.0 * math.pi) - torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1)
                - 0.5 * (y * y).sum(-1))

    def _sample(self, n_samples=1, **kwargs):
        K = int(n_samples)
        lead = (K,) if K > 1 else ()
        batch = tuple(self._batch)
        D = self._n_dims
        eps, seed, call, rng_state = self._noise(lead + batch + (D,))
        if D > _mvn_hip.MAX_DIM:
            if eps is None:
                eps = _ops.philox_normal(lead + batch + (D,), self._mean.device, seed, call, rng_state, self._dtype)
            L = torch.tril(self._cov_tril)
            z = self._mean + (L @ eps[..., None])[..., 0]
            if self._is_reparameterized:
                lp = (-0.5 * D * math.log(2.0 * math.pi) - torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1)
                      - 0.5 * (eps * eps).sum(-1)).expand(lead + batch)
                note_path(self, "torch composition (matmul; the density of the draw needs no solve)", WIDE)
            else:          # the draw is a constant: the density keeps its direct dependence on the parameters
                z = z.detach()
                lp = self._torch_log_prob(self._mean, self._cov_tril, z).expand(lead + batch)
                note_path(self, "torch composition (matmul, solve_triangular at the detached draw)", WIDE)
        else:
            mean, tril = self._flat_params(batch)
            z, lp = _F.MvnSampleLogProb.apply(mean, tril, eps, seed, call, rng_state, K, bool(self._is_reparameterized))
            note_path(self, "V1 zs_mvn_sample_logprob: the draw and its log-density in one launch")
            z, lp = z.reshape(lead + batch + (D,)), lp.reshape(lead + batch)
        self.sample_cache = z
        self._fused = (z, lp, 0)
        return z

    def _log_prob_sum(self, given=None, n_fold=0):
        x = self.sample_cache if given is None else given
        if x is None:
            raise RuntimeError("MultivariateNormalCholesky.log_prob(None) needs a cached sample: call sample() first")
        if self._fused is not None and self._fused[0] is x:
            return sum_trailing(self._fused[1], n_fold)
        x = torch.as_tensor(x, dtype=self._dtype).to(self._mean.device)
        D = self._n_dims
        if x.dim() < 1 or x.shape[-1] != D:
            raise ValueError("the last axis of the value must have %d entries, got shape %s" % (D, tuple(x.shape)))
        batch = tuple(self._batch)
        full = tuple(broadcast_shapes(tuple(x.shape[:-1]), batch))
        if D > _mvn_hip.MAX_DIM:
            lp = self._torch_log_prob(self._mean, self._cov_tril, x).expand(full)
            note_path(self, "torch composition (solve_triangular)", WIDE)
            return sum_trailing(lp, n_fold)
        tail = full[len(full) - len(batch):]
        lead = full[:len(full) - len(batch)]
        K, R = _numel(lead), _numel(tail)
        if fold_particles(K, R, D):
            K, R, tail = 1, K * R, full
        rows = x.expand(full + (D,)).reshape(K, R, D).contiguous()
        mean, tril = self._flat_params(tail)
        lp = _F.MvnLogProb.apply(mean, tril, rows, K)
        note_path(self, "V2 zs_mvn_logprob: the log-density of a given value in one launch (forward substitution)")
        return sum_trailing(lp.reshape(full), n_fold)
