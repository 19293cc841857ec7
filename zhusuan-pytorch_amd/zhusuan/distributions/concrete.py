"""ExpConcrete and Concrete, the Gumbel-softmax relaxations of OnehotCategorical (upstream ZhuSuan's
``multivariate.ExpConcrete`` / ``Concrete``; Maddison et al. 2017; the PyTorch reference has neither).  The draw and its
log-density come from the fused HIP kernel C3, the density of a given value from C4 (include/zs_cat.h): one launch each way."""
import torch

from .base import Distribution
from .categorical import _numel, fold_particles, noise_for, sum_trailing
from .utils import assert_same_log_float_dtype
from . import _cat_functions as _F
from .. import _hip
from .._shapes import broadcast_shapes
from ..utils import note_path

__all__ = ['ExpConcrete', 'Concrete', 'ExpGumbelSoftmax', 'GumbelSoftmax']


def _capturing(device):
    return device.type == "cuda" and torch.cuda.is_current_stream_capturing()


class ExpConcrete(Distribution):
    """
    :param temperature: a positive Python number or 0-dim tensor, read ONCE at construction (a tensor is read from its device,
        which a stream capture forbids: RuntimeError); not differentiable.  ValueError when it is not > 0.
    :param logits: float tensor ``[..., N]``, unnormalised log-probabilities; ``batch_shape = logits.shape[:-1]``.
    :param is_reparameterized: False detaches the draw (its log-density keeps the direct dependence on ``logits``).
    Samples are log-probability vectors ``y`` (``logsumexp(y) = 0``) of shape ``[K] + batch_shape + [N]``.
    """
    _event_ndims = 1
    _nonreparam_draw_has_zero_grad = True
    _exp_space = False

    def __init__(self, temperature, logits, dtype=None, is_reparameterized=True, use_path_derivative=False, group_ndims=0,
                 device=None, **kwargs):
        device = _hip.resolve_device(device, logits)
        self._logits = torch.as_tensor(logits, dtype=dtype).to(device)
        dtype = assert_same_log_float_dtype([(self._logits, type(self).__name__ + ".logits")])
        if self._logits.dim() < 1 or self._logits.shape[-1] < 1:
            raise ValueError("logits must have a last axis of at least one category")
        if isinstance(temperature, torch.Tensor):
            if temperature.dim() != 0:
                raise ValueError("temperature must be a scalar")
            if _capturing(temperature.device):
                raise RuntimeError("%s: a tensor temperature is read from its device at construction, which cannot be done while "
                                   "a stream is being captured; pass a Python number" % type(self).__name__)
        self._temperature = float(temperature)
        if not (self._temperature > 0.0 and self._temperature < float("inf")):
            raise ValueError("temperature must be positive, got %r" % (self._temperature,))
        if use_path_derivative:
            raise NotImplementedError("%s: use_path_derivative is not implemented (the density of the node's own draw comes "
                                      "out of the sampling kernel together with the draw)" % type(self).__name__)
        self._n_categories = int(self._logits.shape[-1])
        super(ExpConcrete, self).__init__(dtype=dtype, is_continuous=True, is_reparameterized=is_reparameterized,
                                          use_path_derivative=use_path_derivative, group_ndims=group_ndims, device=device, **kwargs)
        self._fused = None          # (sample tensor, its log-density over the batch shape, 0)
        self.last_path = None          # which kernel the last sample / log_prob ran on (zhusuan.explain)

    @property
    def temperature(self):
        return self._temperature

    @property
    def logits(self):
        return self._logits

    @property
    def n_categories(self):
        return self._n_categories

    def _batch_shape(self):
        return torch.Size(self._logits.shape[:-1])

    def _flat_logits(self, batch=None):
        lg = self._logits if batch is None else self._logits.expand(tuple(batch) + (self._n_categories,))
        return lg.reshape(-1, self._n_categories).contiguous()

    def _sample(self, n_samples=1, **kwargs):
        K = int(n_samples)
        lead = (K,) if K > 1 else ()
        batch = tuple(self._batch_shape())
        u, seed, call, rng_state = noise_for(lead + tuple(self._logits.shape), self._logits)
        y, ey, lp = _F.RelaxedSampleLogProb.apply(self._flat_logits(), u, seed, call, rng_state, K, self._temperature,
                                                  self._exp_space, bool(self._is_reparameterized))
        note_path(self, "C3 zs_cat_expconcrete_sample_logprob: the relaxed draw and its log-density in one launch")
        z = (ey if self._exp_space else y).reshape(lead + batch + (self._n_categories,))
        self.sample_cache = z
        self._fused = (z, lp.reshape(lead + batch), 0)
        return z

    def _to_log_space(self, x):
        return x

    def _log_prob_sum(self, given=None, n_fold=0):
        x = self.sample_cache if given is None else given
        if x is None:
            raise RuntimeError("%s.log_prob(None) needs a cached sample: call sample() first" % type(self).__name__)
        if self._fused is not None and self._fused[0] is x:
            return sum_trailing(self._fused[1], n_fold)
        x = torch.as_tensor(x, dtype=self._dtype).to(self._logits.device)
        N = self._n_categories
        if x.dim() < 1 or x.shape[-1] != N:
            raise ValueError("the last axis of the value must have %d entries, got shape %s" % (N, tuple(x.shape)))
        batch = tuple(self._batch_shape())
        full = tuple(broadcast_shapes(tuple(x.shape[:-1]), batch))
        tail = full[len(full) - len(batch):]
        K, R = _numel(full[:len(full) - len(batch)]), _numel(tail)
        y = self._to_log_space(x)
        if tuple(y.shape) != full + (N,):
            y = y.expand(full + (N,))
        if fold_particles(K, R, N):
            K, R, tail = 1, K * R, full
        lp = _F.RelaxedLogProb.apply(self._flat_logits(tail if tail != batch else None), y.reshape(K, R, N).contiguous(), K,
                                     self._temperature, self._exp_space)
        note_path(self, "C4 zs_cat_expconcrete_logprob: the log-density of a given value in one launch")
        return sum_trailing(lp.reshape(full), n_fold)


class Concrete(ExpConcrete):
    """The same relaxation in probability space: samples are points of the simplex, ``exp`` of an ExpConcrete draw, written by
    the same launch; the density is that of ExpConcrete minus ``sum_j log x_j``.  ``log_prob`` of a value that is not the node's
    own draw takes ``log(given)`` in torch first."""
    _exp_space = True

    def _to_log_space(self, x):
        return torch.log(x)


ExpGumbelSoftmax = ExpConcrete
GumbelSoftmax = Concrete
