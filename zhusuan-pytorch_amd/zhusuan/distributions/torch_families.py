"""The six families the reference wraps around ``torch.distributions`` -- Beta, Exponential, Gamma, Laplace, Poisson,
StudentT (zhusuan/distributions/{beta,exponential,gamma,laplace,poisson,studentT}.py) -- as thin PASS-THROUGHS.

They are off the variational-inference hot path named by BASELINE.json: no HIP kernel
is written for them and none is claimed.  They exist so that model code written against the reference keeps working after
the switch: sampling and log-prob are exactly the reference's ``torch.distributions`` calls (on whatever device the
parameters live on), with the reference's conventions -- parameters repeated along a leading sample axis, never
reparameterised (``sample()``, not ``rsample()``), ``sample_cache``, the group sum of ``Distribution.log_prob``.
One generic implementation instead of six files.  ``FlowDistribution`` (flow_distribution.py) lives here too: a base
distribution seen through a ``zhusuan.invertible`` network, its log-density tail on the kernels of include/zs_flow.h.
"""
import warnings

import torch

from .base import Distribution
from .utils import assert_same_log_float_dtype, check_broadcast
from .. import _hip
from .._shapes import broadcast_shapes

__all__ = ['Beta', 'Exponential', 'Gamma', 'Laplace', 'Poisson', 'StudentT', 'FlowDistribution']

_INT2FLOAT = {torch.int8: torch.float16, torch.int16: torch.float16, torch.int32: torch.float32, torch.int64: torch.float64,
              torch.uint8: torch.float16}


def _repeat_like_reference(p, n_samples, anchor_ndim):
    """``p.repeat([n_samples, 1, ..., 1])`` with one 1 per axis of the family's ANCHOR parameter (e.g. beta.py:50-54:
    ``_len = len(self._alpha.shape)`` serves alpha and beta alike): a leading sample axis, lower-rank parameters padded."""
    return p.repeat([n_samples] + [1] * anchor_ndim)


class _TorchFamily(Distribution):
    """Generic pass-through: subclasses name the torch class, the parameters (in the reference's argument order) and
    their defaults."""
    _torch_cls = None
    _params = ()              # ((name, default or _REQUIRED), ...)
    _int_rate_ok = False      # Poisson: an integer rate is converted with a warning (poisson.py:29-31)
    _anchor = None            # the parameter whose rank decides the repeat pattern and the "has a sample axis" test

    def __init__(self, *args, dtype=None, is_continuous=True, group_ndims=0, device=None, **kwargs):
        names = [n for n, _ in self._params]
        if len(args) > len(names):
            raise TypeError("%s takes at most %d positional parameters" % (type(self).__name__, len(names)))
        given = dict(zip(names, args))
        for n, default in self._params:
            if n in kwargs:
                if n in given:
                    raise TypeError("%s got multiple values for argument '%s'" % (type(self).__name__, n))
                given[n] = kwargs.pop(n)
            elif n not in given:
                if default is _REQUIRED:
                    raise TypeError("%s missing required argument '%s'" % (type(self).__name__, n))
                given[n] = default
        device = _hip.resolve_device(device, *[given[n] for n in names])
        vals = []
        for n in names:
            v = torch.as_tensor(given[n], dtype=dtype).to(device)
            if self._int_rate_ok and v.dtype in _INT2FLOAT:
                warnings.warn("the tensor dtype convert %s to  %s" % (v.dtype, _INT2FLOAT[v.dtype]))
                v = torch.as_tensor(v, dtype=_INT2FLOAT[v.dtype])
            vals.append(v)
        for a, b in zip(vals, vals[1:]):
            check_broadcast(a, b)
        dtype = assert_same_log_float_dtype([(v, "%s.%s" % (type(self).__name__, n)) for n, v in zip(names, vals)])
        for n, v in zip(names, vals):
            setattr(self, "_" + n, v)
        # the reparameterisation trick is not applied for these families (e.g. exponential.py:27-29)
        super(_TorchFamily, self).__init__(dtype, is_continuous, is_reparameterized=False, group_ndims=group_ndims,
                                           device=device, **kwargs)

    def _values(self):
        return [getattr(self, "_" + n) for n, _ in self._params]

    def _batch_shape(self):
        return torch.Size(broadcast_shapes(*[v.shape for v in self._values()]))

    def _sample(self, n_samples=1, **kwargs):
        vals = self._values()
        if n_samples > 1:
            nd = getattr(self, "_" + self._anchor).dim()
            vals = [_repeat_like_reference(v, n_samples, nd) for v in vals]
        s = self._torch_cls(*vals).sample()
        self.sample_cache = s
        return s

    def _log_prob_sum(self, given=None, n_fold=0):
        x = self.sample_cache if given is None else given
        if x is None:
            raise RuntimeError("%s.log_prob(None) needs a cached sample: call sample() first" % type(self).__name__)
        vals = self._values()
        nd = getattr(self, "_" + self._anchor).dim()
        if x.dim() > nd:
            vals = [_repeat_like_reference(v, x.shape[0], nd) for v in vals]
        lp = self._torch_cls(*vals).log_prob(x)
        if n_fold > 0:
            lp = lp.sum(tuple(range(lp.dim() - n_fold, lp.dim())))
        return lp


_REQUIRED = object()


def _family(name, torch_cls, params, doc, int_rate_ok=False, anchor=None):
    ns = {"_torch_cls": torch_cls, "_params": tuple(params), "_int_rate_ok": int_rate_ok, "__doc__": doc,
          "_anchor": anchor or params[0][0]}
    for n, _ in params:
        ns[n] = property(lambda self, _n=n: getattr(self, "_" + _n))
    return type(name, (_TorchFamily,), ns)


Beta = _family('Beta', torch.distributions.beta.Beta, [("alpha", _REQUIRED), ("beta", _REQUIRED)],
               "Beta(alpha, beta): pass-through of torch.distributions.Beta (zhusuan/distributions/beta.py).")
Exponential = _family('Exponential', torch.distributions.exponential.Exponential, [("rate", _REQUIRED)],
                      "Exponential(rate): pass-through of torch.distributions.Exponential (exponential.py).")
Gamma = _family('Gamma', torch.distributions.gamma.Gamma, [("alpha", _REQUIRED), ("beta", _REQUIRED)],
                "Gamma(alpha, beta): concentration alpha, rate beta; pass-through of torch.distributions.Gamma (gamma.py).")
Laplace = _family('Laplace', torch.distributions.laplace.Laplace, [("loc", _REQUIRED), ("scale", _REQUIRED)],
                  "Laplace(loc, scale): pass-through of torch.distributions.Laplace (laplace.py).", anchor="loc")
Poisson = _family('Poisson', torch.distributions.poisson.Poisson, [("rate", _REQUIRED)],
                  "Poisson(rate): pass-through of torch.distributions.Poisson (poisson.py).", int_rate_ok=True)
StudentT = _family('StudentT', torch.distributions.studentT.StudentT, [("df", _REQUIRED), ("loc", 0.), ("scale", 1.)],
                   "StudentT(df, loc=0, scale=1): pass-through of torch.distributions.StudentT (studentT.py).", anchor="loc")


class FlowDistribution(Distribution):
    """A distribution defined by a latent (base) distribution and an invertible network
    (zhusuan/distributions/flow_distribution.py:10-51 of the reference).

    ``sample(n)`` draws from ``latents`` and runs the transformation with ``reverse=True``; ``n_samples=-1`` returns
    ``None`` (no sample: the node is only scored, as ``self.sn(flow_dis, name="x", n_samples=-1)`` does inside a
    ``BayesianNet``).  ``log_prob(x)`` runs the transformation forward and returns ``sum_dim1 log p(z) + log_det_J``.

    For a ``Normal`` or ``Logistic`` base whose parameters do not require grad and are ``[D]`` or ``[B, D]``, with a
    log-det that is absent, a scalar or ``[B]``, the log-density, the row sum and the add are ONE launch
    (``zs_flow_tail``; its backward another); any other base calls ``latents.log_prob``, ``torch.sum(dim=1)`` and the add as
    the reference does.  ``zhusuan.explain`` / ``last_path`` say which ran.  A ``[B, D]`` log-det, as from a bare ``MADE``,
    fails in the add as in the reference.

    :param latents: an instance of ``Distribution``, the base of the flow.
    :param transformation: a ``zhusuan.invertible.RevNet``; only those are supported.
    :param flow_kwargs: additional info to be recorded.
    """

    def __init__(self, latents, transformation, flow_kwargs=None, dtype=torch.float32, group_ndims=0, device=None, **kwargs):
        from ..invertible.base import RevNet
        if not isinstance(transformation, RevNet) or not isinstance(latents, Distribution):
            raise NotImplementedError(
                "zhusuan.distributions.FlowDistribution: only a zhusuan.distributions.Distribution as `latents` and a "
                "zhusuan.invertible.RevNet as `transformation` are supported; anything else is outside the "
                "variational-inference hot path of the MI355X build")
        self._latents = latents
        self._transformation = transformation
        self._flow_kwargs = flow_kwargs
        self.last_path = None
        if device is None:
            device = latents.device
        super(FlowDistribution, self).__init__(dtype=dtype, is_continuous=True, is_reparameterized=False,
                                               group_ndims=group_ndims, device=device, **kwargs)

    @property
    def latents(self):
        return self._latents

    @property
    def transformation(self):
        return self._transformation

    def _batch_shape(self):
        return self._latents.batch_shape

    def _sample(self, n_samples=-1, **kwargs):
        if n_samples == -1:          # no sample (flow_distribution.py:43-44)
            return None
        z = self._latents.sample(n_samples)
        x, _ = self._transformation.forward(z, reverse=True, **kwargs)
        return x

    def _fused_tail_operands(self, z, log_det):
        """(base, loc, scale, param_rows, logdet, kind) when the one-launch tail takes this call, else a reason."""
        from .normal import Normal
        from .logistic import Logistic
        from .. import _flow_hip
        lat = self._latents
        if type(lat) is Normal:
            base, loc, scale = _flow_hip.NORMAL, lat._mean, lat.std
        elif type(lat) is Logistic:
            base, loc, scale = _flow_hip.LOGISTIC, lat._loc, lat._scale
        else:
            return "the base is a %s (the fused tail takes Normal and Logistic)" % type(lat).__name__
        if lat.group_ndims != 0:
            return "the base sums over group_ndims itself"
        if not isinstance(z, torch.Tensor) or z.dim() != 2 or z.dtype not in (torch.float32, torch.float64):
            return "the transformed value is not a float [B, D] tensor"
        if loc.requires_grad or scale.requires_grad:
            return "a parameter of the base requires grad"
        B, D = z.shape
        if tuple(loc.shape) != tuple(scale.shape) or tuple(loc.shape) not in ((D,), (B, D)):
            return "the base's parameters are neither [D] nor [B, D]"
        if loc.dtype != z.dtype or loc.device != z.device or scale.device != z.device:
            return "the base's parameters and the value differ in dtype or device"
        if log_det is None:
            kind = _flow_hip.LOGDET_NONE
        elif not isinstance(log_det, torch.Tensor) or log_det.dtype != z.dtype or log_det.device != z.device:
            return "the log-det is not a tensor of the value's dtype and device"
        elif log_det.numel() == 1 and log_det.dim() <= 1:
            kind = _flow_hip.LOGDET_SCALAR
        elif tuple(log_det.shape) == (B,):
            kind = _flow_hip.LOGDET_ROWS
        else:
            return "the log-det has shape %s" % (tuple(log_det.shape),)
        return base, loc.contiguous(), scale.contiguous(), int(loc.dim() == 2), log_det, kind

    def _log_prob(self, *given, **kwargs):
        from ..utils import note_path
        z, log_det_J = self._transformation.forward(*given, **kwargs, reverse=False)
        plan = self._fused_tail_operands(z, log_det_J)
        if not isinstance(plan, str):
            from ..invertible import _functions as F
            base, loc, scale, rows, ld, kind = plan
            out = F.Tail.apply(z.contiguous(), loc, scale, None if ld is None else ld.contiguous(), base, rows, kind)
            if kind == 1 and ld.dim() == 1:          # ([B] + [1] broadcasts to [B] in the reference as well)
                out = out.reshape(torch.broadcast_shapes(out.shape, ld.shape))
            note_path(self, "F-tail: base log-density, row sum and log-det add in one launch each way (zs_flow_tail)")
            return out
        note_path(self, "reference ops: latents.log_prob, torch.sum(dim=1), add", plan)
        log_ll = torch.sum(self._latents.log_prob(z), dim=1)
        return log_ll + log_det_J

    def _log_prob_sum(self, given=None, n_fold=0):
        x = self.sample_cache if given is None else given
        if x is None:
            raise RuntimeError("FlowDistribution.log_prob(None) needs a value: observe the node or pass one")
        lp = self._log_prob(x)
        if n_fold > 0:
            lp = lp.sum(tuple(range(lp.dim() - n_fold, lp.dim())))
        return lp
