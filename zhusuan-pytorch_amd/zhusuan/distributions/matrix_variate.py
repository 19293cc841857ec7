"""MatrixVariateNormalCholesky (upstream ZhuSuan's ``multivariate.MatrixVariateNormalCholesky``; the PyTorch reference dropped
it): a normal over ``n x p`` matrices with mean ``mean``, row covariance ``U U^T`` and column covariance ``V V^T``, ``U = u_tril``
and ``V = v_tril`` lower triangular -- ``vec`` of a draw (rows first) has covariance ``kron(U U^T, V V^T)``.  The posterior of the
matrix-variate-Gaussian Bayesian networks: correlated weights for ``n^2 + p^2`` parameters.

With ``n`` and ``p`` up to 128 (float32) or 64 (float64), on a HIP device, the draw and its log-density come from the fused
matrix-core kernel M1, the density of a given value from M2 (include/zs_matvar.h): one launch each, a main and a finish launch
for the backwards.  Wider events, and CPU tensors, run the torch composition; ``last_path`` / ``zhusuan.explain`` say which."""
import torch

from .base import Distribution
from .categorical import _numel, sum_trailing
from .utils import assert_same_log_float_dtype
from . import _matvar_functions as _F
from .. import _hip, _ops, _rng
from .._shapes import broadcast_shapes
from ..utils import note_path

__all__ = ['MatrixVariateNormalCholesky']


def fold_particles(K, R):
    """Whether a given value of K particles over R rows goes to the kernels as K R rows of one particle (parameters expanded).
    The backward kernels cut a row's particles into ``shares(K, R)`` contiguous shares, one workgroup each (include/zs_matvar.h).
    Where that leaves a workgroup walking several particles in turn while the launch is still short of the workgroups the split
    aims for -- one weight matrix against a batch of 50 observations runs on 13 -- the value is folded: every event gets its own
    workgroup, and autograd sums the expanded parameters' gradient (which costs ``[K R, n, n]`` and ``[K R, p, p]`` expansions).
    The rule follows the kernels' own split; where the crossover in time lies has not been measured.  The node's own draw (M1) is
    not folded: its K particles over few rows keep the share split."""
    s = _F.shares(K, R)
    return K > s and s * R < _F.GRID_TARGET


class MatrixVariateNormalCholesky(Distribution):
    """
    :param mean: float tensor ``[..., n, p]``.
    :param u_tril: float tensor ``[..., n, n]``, the lower-triangular Cholesky factor of the covariance among the rows.
    :param v_tril: float tensor ``[..., p, p]``, the lower-triangular Cholesky factor of the covariance among the columns.
        Only the lower triangles are read (the gradients' upper triangles are zero); the diagonals must be positive, which is not
        checked: a zero or negative entry gives ``-inf`` / NaN log-densities.
    :param is_reparameterized: False detaches the draw (its log-density keeps the direct dependence on the parameters).
    ``batch_shape`` is the broadcast of ``mean.shape[:-2]``, ``u_tril.shape[:-2]`` and ``v_tril.shape[:-2]``; samples are
    ``[K] + batch_shape + [n, p]``.
    """
    _event_ndims = 2
    _nonreparam_draw_has_zero_grad = True

    def __init__(self, mean, u_tril, v_tril, dtype=None, is_reparameterized=True, use_path_derivative=False, group_ndims=0,
                 device=None, **kwargs):
        device = _hip.resolve_device(device, mean, u_tril, v_tril)
        self._mean = torch.as_tensor(mean, dtype=dtype).to(device)
        self._u_tril = torch.as_tensor(u_tril, dtype=dtype).to(device)
        self._v_tril = torch.as_tensor(v_tril, dtype=dtype).to(device)
        dtype = assert_same_log_float_dtype([(self._mean, 'MatrixVariateNormalCholesky.mean'),
                                             (self._u_tril, 'MatrixVariateNormalCholesky.u_tril'),
                                             (self._v_tril, 'MatrixVariateNormalCholesky.v_tril')])
        if self._mean.dim() < 2 or self._mean.shape[-2] < 1 or self._mean.shape[-1] < 1:
            raise ValueError("mean must have shape [..., n, p] with n, p >= 1, got %s" % (tuple(self._mean.shape),))
        n, p = int(self._mean.shape[-2]), int(self._mean.shape[-1])
        if self._u_tril.dim() < 2 or tuple(self._u_tril.shape[-2:]) != (n, n):
            raise ValueError("u_tril must have shape [..., %d, %d] (mean %s has %d rows), got %s"
                             % (n, n, tuple(self._mean.shape), n, tuple(self._u_tril.shape)))
        if self._v_tril.dim() < 2 or tuple(self._v_tril.shape[-2:]) != (p, p):
            raise ValueError("v_tril must have shape [..., %d, %d] (mean %s has %d columns), got %s"
                             % (p, p, tuple(self._mean.shape), p, tuple(self._v_tril.shape)))
        leads = [tuple(t.shape[:-2]) for t in (self._mean, self._u_tril, self._v_tril)]
        try:
            self._batch = torch.Size(broadcast_shapes(broadcast_shapes(leads[0], leads[1]), leads[2]))
        except RuntimeError as e:
            raise ValueError("the batch shapes of mean %s, u_tril %s and v_tril %s do not broadcast: %s" % (tuple(leads) + (e,)))
        if use_path_derivative:
            raise NotImplementedError("MatrixVariateNormalCholesky: use_path_derivative is not implemented (the density of the "
                                      "node's own draw comes out of the sampling kernel together with the draw)")
        self._n, self._p = n, p
        super(MatrixVariateNormalCholesky, self).__init__(dtype=dtype, is_continuous=True, is_reparameterized=is_reparameterized,
                                                          use_path_derivative=use_path_derivative, group_ndims=group_ndims,
                                                          device=device, **kwargs)
        self._fused = None          # (sample tensor, its log-density over the batch shape, 0)
        self.last_path = None          # which path the last sample / log_prob ran on (zhusuan.explain)

    @property
    def mean(self):
        return self._mean

    @property
    def u_tril(self):
        return self._u_tril

    @property
    def v_tril(self):
        return self._v_tril

    def _batch_shape(self):
        return self._batch

    def _off_kernels(self):
        """Why the kernels do not take this node, or None."""
        cap = _F.MAX_DIM[self._mean.element_size()]
        if self._mean.device.type != "cuda":
            return "the operands are on the CPU"
        if self._n > cap or self._p > cap:
            return ("events with more than %d rows or columns (%s) are outside the fused kernels' domain (zs_matvar_max_dim)"
                    % (cap, str(self._dtype).replace("torch.", "")))
        return None

    def _flat_params(self, batch):
        """(mean [R, n, p], u [R, n, n], v [R, p, p]) expanded to ``batch`` and contiguous; autograd sums the expanded gradient."""
        n, p = self._n, self._p
        batch = tuple(batch)
        return (self._mean.expand(batch + (n, p)).reshape(-1, n, p).contiguous(),
                self._u_tril.expand(batch + (n, n)).reshape(-1, n, n).contiguous(),
                self._v_tril.expand(batch + (p, p)).reshape(-1, p, p).contiguous())

    def _noise(self, shape):
        """(eps, seed, call, rng_state) of one draw: the injected / reference-stream normals, else the next Philox call."""
        eps = _rng.pop_injected(shape, self._mean.device, self._dtype, kind="normal")
        if eps is not None:
            return eps.contiguous(), 0, 0, None
        if self._mean.device.type != "cuda":
            return torch.randn(shape, dtype=self._dtype, device=self._mean.device), 0, 0, None
        seed, call, rng_state = _rng.next_call(self._mean.device)
        return None, seed, call, rng_state

    def _sample(self, n_samples=1, **kwargs):
        K = int(n_samples)
        lead = (K,) if K > 1 else ()
        batch = tuple(self._batch)
        n, p = self._n, self._p
        eps, seed, call, rng_state = self._noise(lead + batch + (n, p))
        why = self._off_kernels()
        if why is not None:
            if eps is None:
                eps = _ops.philox_normal(lead + batch + (n, p), self._mean.device, seed, call, rng_state, self._dtype)
            z, lp = _F.torch_sample(self._mean, self._u_tril, self._v_tril, eps)
            if self._is_reparameterized:
                note_path(self, "torch composition (matmul; the density of the draw needs no solve)", why)
            else:          # the draw is a constant: the density keeps its direct dependence on the parameters
                z = z.detach()
                lp = _F.torch_log_prob(self._mean, self._u_tril, self._v_tril, z)
                note_path(self, "torch composition (matmul, solve_triangular at the detached draw)", why)
            lp = lp.expand(lead + batch)
        else:
            mean, u, v = self._flat_params(batch)
            z, lp = _F.MatvarSampleLogProb.apply(mean, u, v, eps, seed, call, rng_state, K, bool(self._is_reparameterized))
            note_path(self, "M1 zs_matvar_sample_logprob: the draw and its log-density in one launch on the matrix cores")
            z, lp = z.reshape(lead + batch + (n, p)), lp.reshape(lead + batch)
        self.sample_cache = z
        self._fused = (z, lp, 0)
        return z

    def _log_prob_sum(self, given=None, n_fold=0):
        x = self.sample_cache if given is None else given
        if x is None:
            raise RuntimeError("MatrixVariateNormalCholesky.log_prob(None) needs a cached sample: call sample() first")
        if self._fused is not None and self._fused[0] is x:
            return sum_trailing(self._fused[1], n_fold)
        x = torch.as_tensor(x, dtype=self._dtype).to(self._mean.device)
        n, p = self._n, self._p
        if x.dim() < 2 or tuple(x.shape[-2:]) != (n, p):
            raise ValueError("the last two axes of the value must be [%d, %d], got shape %s" % (n, p, tuple(x.shape)))
        batch = tuple(self._batch)
        full = tuple(broadcast_shapes(tuple(x.shape[:-2]), batch))
        why = self._off_kernels()
        if why is not None:
            lp = _F.torch_log_prob(self._mean, self._u_tril, self._v_tril, x).expand(full)
            note_path(self, "torch composition (solve_triangular from the left and from the right)", why)
            return sum_trailing(lp, n_fold)
        tail = full[len(full) - len(batch):]
        lead = full[:len(full) - len(batch)]
        K, R = _numel(lead), _numel(tail)
        if fold_particles(K, R):
            K, R, tail = 1, K * R, full
        rows = x.expand(full + (n, p)).reshape(K, R, n, p).contiguous()
        mean, u, v = self._flat_params(tail)
        lp = _F.MatvarLogProb.apply(mean, u, v, rows, K)
        note_path(self, "M2 zs_matvar_logprob: the log-density of a given value in one launch (blocked substitution on the matrix cores)")
        return sum_trailing(lp.reshape(full), n_fold)
