"""NormalMixture: a mixture of C diagonal Gaussians over D-vectors,

    log_prob(x) = logsumexp_c( log_softmax(logits)_c + sum_d log N(x_d; mean_cd, std_cd) ),

the learned prior of a VAE (a mixture-of-Gaussians prior; the VampPrior of Tomczak & Welling 2018 when ``mean, logstd =
encoder(pseudo_inputs)``) or a GMM likelihood.  For events up to 64 wide on a HIP device the value and the gradients for ``x``,
``logits``, ``mean`` and ``logstd`` / ``std`` come from the fused matrix-core kernels of include/zs_mix.h; wider events, CPU
tensors and values without rows run the torch composition (the same matmul form); ``last_path`` / ``zhusuan.explain`` say
which.  What the kernel path saves is memory: nothing of size ``[rows, C]`` or ``[rows, C, D]`` is allocated or kept for the
backward (DESIGN.md 4o has the measured times, the ones behind torch included)."""
import torch

from .base import Distribution
from .categorical import Categorical, _numel, sum_trailing
from .normal import Normal
from .utils import assert_same_log_float_dtype
from . import _mix_functions as _F
from .. import _hip
from ..utils import note_path

__all__ = ['NormalMixture']

KERNELS = ("zs_mix_prepare + zs_mix_logprob: the score tiles in matrix-core accumulators, online logsumexp; "
           "zs_mix_grad_x / zs_mix_grad_params backward")
COMPOSITION = "torch composition (matmul of [y | y^2] with the packed components, logsumexp)"


class NormalMixture(Distribution):
    """
    :param logits: float tensor ``[C]``, the unnormalised log-weights of the components.
    :param mean: float tensor ``[C, D]``.
    :param std / logstd: float tensor ``[C, D]``; exactly one of them (ValueError otherwise, as ``Normal``).
    :param batch_shape: the shape of one draw without its event axis: ``sample(n)`` is ``[n] + batch_shape + [D]``.  The
        parameters are shared by the whole batch.
    An event is a D-vector.  ``log_prob(x)`` takes ``x`` of any shape ``[..., D]`` and returns ``x.shape[:-1]`` (``group_ndims``
    folds trailing axes of that).  Never reparameterised: a draw is detached from the parameters.
    """
    _event_ndims = 1
    _nonreparam_draw_has_zero_grad = True

    def __init__(self, logits, mean, std=None, logstd=None, batch_shape=(), dtype=None, group_ndims=0, device=None, **kwargs):
        device = _hip.resolve_device(device, logits, mean, std, logstd)
        if (logstd is None) == (std is None):
            raise ValueError("Either `std` or `logstd` should be passed. It is not allowed "
                             "that both are specified or both are not.")
        self._logits = torch.as_tensor(logits, dtype=dtype).to(device)
        self._mean = torch.as_tensor(mean, dtype=dtype).to(device)
        self._std_given = None if std is None else torch.as_tensor(std, dtype=dtype).to(device)
        self._logstd_given = None if logstd is None else torch.as_tensor(logstd, dtype=dtype).to(device)
        scale, scale_name = (self._std_given, 'std') if logstd is None else (self._logstd_given, 'logstd')
        dtype = assert_same_log_float_dtype([(self._logits, 'NormalMixture.logits'), (self._mean, 'NormalMixture.mean'),
                                             (scale, 'NormalMixture.' + scale_name)])
        if self._logits.dim() != 1 or self._logits.shape[0] < 1:
            raise ValueError("logits must have shape [C] with at least one component, got %s" % (tuple(self._logits.shape),))
        C = int(self._logits.shape[0])
        if self._mean.dim() != 2 or self._mean.shape[0] != C or self._mean.shape[1] < 1:
            raise ValueError("mean must have shape [%d, D] (logits %s has %d components), got %s"
                             % (C, tuple(self._logits.shape), C, tuple(self._mean.shape)))
        if tuple(scale.shape) != tuple(self._mean.shape):
            raise ValueError("%s must have the shape of mean %s, got %s" % (scale_name, tuple(self._mean.shape), tuple(scale.shape)))
        self._n_components, self._n_dims = C, int(self._mean.shape[1])
        self._batch = torch.Size(tuple(int(s) for s in batch_shape))
        super(NormalMixture, self).__init__(dtype=dtype, is_continuous=True, is_reparameterized=False, group_ndims=group_ndims,
                                            device=device, **kwargs)
        self.last_path = None          # which path the last log_prob ran on (zhusuan.explain)
        self.last_workspaces = {}      # filled by the kernel path's backward: which gradient launches ran, the size of the partials

    @property
    def logits(self):
        return self._logits

    @property
    def mean(self):
        return self._mean

    @property
    def std(self):
        return torch.exp(self._logstd_given) if self._std_given is None else self._std_given

    @property
    def logstd(self):
        return torch.log(self._std_given) if self._logstd_given is None else self._logstd_given          # (the chain rule of std=)

    @property
    def n_components(self):
        return self._n_components

    @property
    def n_dims(self):
        return self._n_dims

    def _batch_shape(self):
        return self._batch

    def _sample(self, n_samples=1, **kwargs):
        """The component index from the Categorical kernels, then ``mean_c + std_c eps`` from the Normal kernels on the gathered
        rows; detached from the parameters."""
        batch, C = tuple(self._batch), self._n_components
        idx = Categorical(self._logits.detach().expand(batch + (C,)), device=self._logits.device).sample(int(n_samples))
        mu = self._mean.detach()[idx]
        if self._std_given is None:
            draw = Normal(mu, logstd=self._logstd_given.detach()[idx], is_reparameterized=False, device=mu.device)
        else:
            draw = Normal(mu, std=self._std_given.detach()[idx], is_reparameterized=False, device=mu.device)
        self.sample_cache = draw.sample().detach()
        return self.sample_cache

    def _log_prob_sum(self, given=None, n_fold=0):
        x = self.sample_cache if given is None else given
        if x is None:
            raise RuntimeError("NormalMixture.log_prob(None) needs a cached sample: call sample() first")
        x = torch.as_tensor(x, dtype=self._dtype).to(self._mean.device)
        C, D = self._n_components, self._n_dims
        if x.dim() < 1 or x.shape[-1] != D:
            raise ValueError("the last axis of the value must have %d entries (mean is %s), got shape %s"
                             % (D, tuple(self._mean.shape), tuple(x.shape)))
        R = _numel(x.shape[:-1])
        logits, mean, logstd = self._logits, self._mean, self.logstd
        why = None
        if mean.device.type != "cuda":
            why = "the operands are on the CPU"
        elif D > _F.MAX_DIM:
            why = "events wider than %d are outside the fused kernels' domain (zs_mix_max_dim)" % _F.MAX_DIM
        elif C > _F.MAX_COMPONENTS:
            why = "more than %d components are outside the fused kernels' domain (zs_mix_max_components)" % _F.MAX_COMPONENTS
        elif R == 0:
            why = "there are no rows"
        if why is not None:
            lp = _F.torch_log_prob(logits, mean, logstd, x)
            note_path(self, COMPOSITION, why)
        else:
            self.last_workspaces = {}
            lp = _F.MixtureLogProb.apply(logits.contiguous(), mean.contiguous(), logstd.contiguous(), x.reshape(R, D).contiguous(),
                                         self.last_workspaces).reshape(x.shape[:-1])
            note_path(self, KERNELS)
        return sum_trailing(lp, n_fold)
