"""Categorical and OnehotCategorical (upstream ZhuSuan's ``univariate.Categorical`` / ``multivariate.OnehotCategorical``; the
PyTorch reference has neither).  The draw (Gumbel-max) and its log-mass come from the fused HIP kernel C1, the log-mass of a
given value from C2 (include/zs_cat.h): one launch each way."""
import torch

from .base import Distribution
from .utils import assert_same_log_float_dtype
from . import _cat_functions as _F
from .. import _hip, _rng
from .._shapes import broadcast_shapes
from ..utils import note_path

__all__ = ['Categorical', 'OnehotCategorical', 'Discrete', 'OnehotDiscrete']


def _numel(shape):
    n = 1
    for s in shape:
        n *= int(s)
    return n


def sum_trailing(lp, n_fold):
    """The sum over the last ``n_fold`` axes of the small ``[K, R]``-sized result: a torch ``sum``."""
    if n_fold > lp.dim():
        raise ValueError("cannot sum %d trailing axes of a result of shape %s" % (n_fold, tuple(lp.shape)))
    return lp.sum(dim=tuple(range(lp.dim() - n_fold, lp.dim()))) if n_fold else lp


def fold_particles(K, R, N):
    """Whether a given value of K particles over R rows goes to the kernels as K R rows of one particle (logits expanded).
    The backward kernels give a lane group a ROW and walk its particles in turn (include/zs_cat.h): with few rows and many
    particles -- logits ``[N]`` against a batch of observations -- they would run on a wave or two.  Rows are cheap to add
    (autograd sums the expanded logits' gradient), so few rows with more than a handful of particles are folded."""
    lanes = 1
    while lanes < 64 and lanes * 4 < N:
        lanes *= 2
    return K > 8 and R * lanes < 4096


def noise_for(shape, logits):
    """(u, seed, call, rng_state) of one draw: the injected / reference-stream uniforms, else the next Philox call."""
    u = _rng.pop_injected(shape, logits.device, logits.dtype, kind="rand")
    if u is not None:
        return u.contiguous(), 0, 0, None
    seed, call, rng_state = _rng.next_call(logits.device)
    return None, seed, call, rng_state


class _CategoricalBase(Distribution):
    _nonreparam_draw_has_zero_grad = True
    _onehot = False

    def __init__(self, logits, dtype=None, group_ndims=0, device=None, **kwargs):
        device = _hip.resolve_device(device, logits)
        self._logits = torch.as_tensor(logits).to(device)
        param_dtype = assert_same_log_float_dtype([(self._logits, type(self).__name__ + ".logits")])
        if self._logits.dim() < 1:
            raise ValueError("logits must have at least one axis (the categories)")
        self._n_categories = int(self._logits.shape[-1])
        if self._n_categories < 1:
            raise ValueError("logits must have at least one category")
        if dtype is None:
            dtype = param_dtype if self._onehot else torch.int64
        elif not self._onehot and (dtype.is_floating_point or dtype == torch.bool):
            raise TypeError("Categorical samples are indices: dtype must be an integer type, got %s" % dtype)
        self._param_dtype = param_dtype
        super(_CategoricalBase, self).__init__(dtype=dtype, is_continuous=False, is_reparameterized=False,
                                               group_ndims=group_ndims, device=device, **kwargs)
        self._fused = None          # (sample tensor, its log-mass over the batch shape, 0)
        self.last_path = None          # which kernel the last sample / log_prob ran on (zhusuan.explain)

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
        idx, onehot, lp = _F.CatSampleLogProb.apply(self._flat_logits(), u, seed, call, rng_state, K, self._onehot)
        note_path(self, "C1 zs_cat_sample_logprob: the Gumbel-max draw and its log-mass in one launch")
        if self._onehot:
            z = onehot.reshape(lead + batch + (self._n_categories,))
        else:
            z = idx.reshape(lead + batch)
        if z.dtype != self._dtype:
            z = z.to(self._dtype)
        self.sample_cache = z
        self._fused = (z, lp.reshape(lead + batch), 0)
        return z

    def _given_rows(self, x):
        """``given`` broadcast against the batch shape: (value as [K, R(, N)] contiguous, K, batch the logits take, full shape)."""
        ev = 1 if self._onehot else 0
        batch = tuple(self._batch_shape())
        vshape = tuple(x.shape)
        if ev:
            if not vshape or vshape[-1] != self._n_categories:
                raise ValueError("the last axis of a one-hot value must have %d entries, got shape %s" % (self._n_categories, vshape))
            vshape = vshape[:-1]
        full = tuple(broadcast_shapes(vshape, batch))
        tail = full[len(full) - len(batch):]
        K, R = _numel(full[:len(full) - len(batch)]), _numel(tail)
        event = (self._n_categories,) if ev else ()
        if tuple(x.shape) != full + event:
            x = x.expand(full + event)
        return x.reshape((K, R) + event).contiguous(), K, tail, full

    def _log_prob_sum(self, given=None, n_fold=0):
        x = self.sample_cache if given is None else given
        if x is None:
            raise RuntimeError("%s.log_prob(None) needs a cached sample: call sample() first" % type(self).__name__)
        if self._fused is not None and self._fused[0] is x:
            return sum_trailing(self._fused[1], n_fold)
        x = torch.as_tensor(x).to(self._logits.device)
        x = x.to(self._param_dtype) if self._onehot else x.to(torch.int64)
        rows, K, tail, full = self._given_rows(x)
        if fold_particles(K, rows.shape[1], self._n_categories):
            rows, K, tail = rows.reshape((1, -1) + tuple(rows.shape[2:])), 1, full
        lp = _F.CatLogProb.apply(self._flat_logits(tail if tail != tuple(self._batch_shape()) else None), rows, K, self._onehot)
        note_path(self, "C2 zs_cat_logprob: the log-mass of a given value in one launch")
        return sum_trailing(lp.reshape(full), n_fold)


class Categorical(_CategoricalBase):
    """
    :param logits: float tensor ``[..., N]``, unnormalised log-probabilities; ``batch_shape = logits.shape[:-1]``.
    :param dtype: the (integer) sample type, default ``torch.int64``.
    Samples are indices in ``[0, N)`` of shape ``[K] + batch_shape``.  Never reparameterised.
    """
    _onehot = False


class OnehotCategorical(_CategoricalBase):
    """
    :param logits: float tensor ``[..., N]``, unnormalised log-probabilities; ``batch_shape = logits.shape[:-1]``.
    :param dtype: the sample type, default that of ``logits``.
    Samples are one-hot vectors of shape ``[K] + batch_shape + [N]``; ``log_prob`` takes any non-negative weights over the last
    axis (``sum_j x_j log softmax(logits)_j``).  Never reparameterised.
    """
    _onehot = True
    _event_ndims = 1


Discrete = Categorical
OnehotDiscrete = OnehotCategorical
