"""The inclusive-KL objective KL(p || q) with self-normalised importance weights: upstream ZhuSuan's ``klpq`` (its ``importance``
estimator, alias ``rws``), the wake-phase update of q in reweighted wake-sleep (Bornschein & Bengio 2015).  The reference this
package follows has no such objective; the interface is that of the two objectives it has (``obj(observed, reduce_mean=True)``).

With K particles z_k ~ q(z | x), log-weights lw_k = log p(x, z_k) - log q(z_k | x) and w_k = softmax_k(lw_k) held constant,

    cost = -sum_k w_k log q(z_k | x)                      gradient for q's parameters: the wake-phase update of q
    cost = -sum_k w_k (log q + log p)(z_k)                ``model_grad=True``: also the wake-phase update of p, in one backward

The weights, the cost, the importance-weighted bound log mean_k exp(lw_k) and the effective sample size 1 / sum_k w_k^2 are ONE
launch (Q1 of include/zs_klpq.h), the gradient w.r.t. every node's log-probability one more; the nodes' own kernels produce the
log-probabilities.  The sleep phase (``sleep_cost``) needs no kernel of its own: it is the variational net's log-probability of
the generator's dreams, which the nodes' kernels already give."""
import math
import warnings

import torch
import torch.nn as nn

from ..framework.stochastic_tensor import StochasticTensor
from .. import _klpq_hip
from .._shapes import broadcast_shapes
from ..utils import note_path as _note_path
from .elbo import latent_value, run_variational
from ._klpq_functions import InclusiveKL, kernel_term

__all__ = ['InclusiveKLObjective', 'KLpq']

_PATH_KERNEL = "Q1: weights, cost, bound and effective sample size in one launch, the gradient of every term in one more (zs_klpq_forward / zs_klpq_backward)"
_PATH_TORCH = "the torch composition of the same formulas (a dozen launches each way)"
_PATH_SINGLE = "-log q of the single sample (torch's additions: there are no weights to form)"
_WARN_SINGLE = ("inclusive KL objective: the self-normalised importance sampling estimator with a single sample is biased; "
                "the cost is -log q of that sample")


def _sum(terms):
    """left to right, as log_joint adds them"""
    total = None
    for t in terms:
        total = t if total is None else total + t
    return total


def torch_composition(terms_p, terms_q, axis, model_grad):
    """(cost, bound, ess) of the header's formulas with torch operations, the particle axis reduced away."""
    lp, lq = _sum(terms_p), _sum(terms_q)
    lw = (lp - lq).detach()
    m = lw.max(axis, keepdim=True).values
    e = torch.exp(lw - m)
    s = e.sum(axis, keepdim=True)
    w = e / s
    x = lq + lp if model_grad else lq
    cost = -torch.where(w == 0, torch.zeros_like(w), w * x).sum(axis)
    bound = (m + torch.log(s)).squeeze(axis) - math.log(lw.shape[axis])
    return cost, bound, 1.0 / (w * w).sum(axis)


def kernel_plan(terms_p, terms_q, axis):
    """The terms as the kernel takes them: ``(terms_p, terms_q, K, B, rest, note)`` -- 2-D ``[K or 1, B or 1]`` tensors (views
    wherever the layout allows), the shape ``rest`` of the non-particle axes, and a note when terms had to be added beforehand
    -- or a string: the reason why this layout runs the torch composition.  ``axis`` is already normalised."""
    every = list(terms_p) + list(terms_q)
    ref = every[0]
    if ref.dtype not in (torch.float32, torch.float64) or any(t.dtype != ref.dtype or t.device != ref.device for t in every):
        return "the log-probabilities are not all float32 or all float64 on one device"
    shape = broadcast_shapes(*[tuple(t.shape) for t in every])
    nd = len(shape)
    if nd > 2 and axis != 0:
        return "the particle axis is not 0 of log-probabilities with more than two axes"
    K = shape[axis]
    rest = tuple(s for i, s in enumerate(shape) if i != axis)
    B = 1
    for s in rest:
        B *= s

    def two_d(t):
        if nd == 2 and axis == 0 and t.dim() == 2:          # already [K or 1, B or 1]: no view, no autograd node
            return kernel_term(t, K, B)
        t = t.reshape((1,) * (nd - t.dim()) + tuple(t.shape)).movedim(axis, 0)
        tail = tuple(t.shape[1:])
        if all(s == 1 for s in tail):
            t = t.reshape(t.shape[0], 1)
        elif tail == rest:
            t = t.reshape(t.shape[0], B)
        else:                                        # shared along some of the batch axes only: spelled out
            t = t.expand((t.shape[0],) + rest).reshape(t.shape[0], B)
        return kernel_term(t, K, B)

    note = None
    sides = []
    for terms in (terms_p, terms_q):
        terms = list(terms)
        if len(terms) > _klpq_hip.MAX_TERMS:
            extra = len(terms) - _klpq_hip.MAX_TERMS + 1
            note = "a side has more than %d terms: its first %d were added with torch beforehand" % (_klpq_hip.MAX_TERMS, extra)
            terms = [_sum(terms[:extra])] + terms[extra:]
        sides.append([two_d(t) for t in terms])
    return sides[0], sides[1], K, B, rest, note


class InclusiveKLObjective(nn.Module):
    """
    :param generator: BayesianNet p(x, z).
    :param variational: BayesianNet q(z | x); its latents must have ``is_reparameterized=False``.
    :param axis: the particle axis of the log-probabilities.  ``None`` (or a single particle) gives upstream's single-sample
        behaviour: a warning, and the cost ``-log q``.
    :param estimator: ``'importance'``; ``'rws'`` is the same thing under its other name.
    :param model_grad: also give the generator's parameters the wake-phase gradient ``-sum_k w_k grad log p(x, z_k)``, so that
        one backward trains both nets (wake-wake).  Without it the generator receives no gradient.

    After a call ``last_iw_bound`` holds the importance-weighted bound per datapoint (detached), ``last_ess`` the effective
    sample size per datapoint, and ``zhusuan.explain(obj)`` says which path ran.
    """

    def __init__(self, generator, variational, axis=None, estimator='importance', model_grad=False):
        super().__init__()
        self.generator = generator
        self.variational = variational
        self._axis = axis
        if estimator not in ['importance', 'rws']:
            raise NotImplementedError()
        self.estimator = estimator
        self.model_grad = bool(model_grad)
        self.last_iw_bound = None
        self.last_ess = None
        self.last_path = None          # which kernels the last evaluation ran on, and why (zhusuan.explain)
        self._warned_single = False

    def forward(self, observed, reduce_mean=True):
        run_variational(self.variational, observed)
        nodes_q = self.variational.nodes
        _v_inputs = {}
        for k, v in nodes_q.items():
            _v_inputs[k] = latent_value(v)
            if isinstance(v, StochasticTensor) and v.dist.is_reparameterized:
                raise ValueError("with importance estimator, the is_reparameterized must be false")
        _observed = {**_v_inputs, **observed}
        nodes_p = self.generator(_observed).nodes
        terms_p = [torch.as_tensor(nodes_p[n].log_prob()) for n in nodes_p.keys()]
        terms_q = [torch.as_tensor(nodes_q[n].log_prob()) for n in nodes_q.keys()]
        return self.importance(terms_p, terms_q, reduce_mean)

    def importance(self, terms_p, terms_q, reduce_mean=True):
        """The objective from the two lists of log-probability tensors (generator, variational), each added left to right."""
        shape = broadcast_shapes(*[tuple(t.shape) for t in list(terms_p) + list(terms_q)])
        nd = len(shape)
        axis = self._axis
        if axis is not None:
            if not -nd <= axis < nd:
                raise IndexError("Dimension out of range (expected to be in range of [%d, %d], but got %d)"
                                 % (-max(nd, 1), max(nd, 1) - 1, axis))
            axis = axis % nd
        if axis is None or shape[axis] == 1:
            return self._single_sample(terms_p, terms_q, axis, reduce_mean)
        plan = kernel_plan(terms_p, terms_q, axis)
        if isinstance(plan, str):
            _note_path(self, _PATH_TORCH, plan)
            cost, bound, ess = torch_composition(terms_p, terms_q, axis, self.model_grad)
            self.last_iw_bound, self.last_ess = bound.detach(), ess.detach()
            return cost.mean() if reduce_mean else cost
        tp, tq, K, B, rest, note = plan
        _note_path(self, _PATH_KERNEL, note)
        cost, bound, ess = InclusiveKL.apply(K, B, len(tp), self.model_grad, bool(reduce_mean), *(tp + tq))
        if len(rest) != 1:
            bound, ess = bound.reshape(rest), ess.reshape(rest)
        self.last_iw_bound, self.last_ess = bound, ess
        return cost if reduce_mean or len(rest) == 1 else cost.reshape(rest)

    rws = importance

    def _single_sample(self, terms_p, terms_q, axis, reduce_mean):
        if not self._warned_single:
            self._warned_single = True
            warnings.warn(_WARN_SINGLE, stacklevel=3)
        _note_path(self, _PATH_SINGLE)
        lp, lq = _sum(terms_p), _sum(terms_q)
        cost = -(lq + lp) if self.model_grad else -lq
        bound = (lp - lq).detach()
        if axis is not None:
            cost, bound = cost.squeeze(axis), bound.squeeze(axis)
        cost = cost.expand(bound.shape)
        self.last_iw_bound, self.last_ess = bound, torch.ones_like(bound)
        return cost.mean() if reduce_mean else cost

    def sleep_cost(self, observed_names, n_samples=None):
        """The sleep phase of reweighted wake-sleep, ``-mean sum log q(z | x)`` at a dream ``(x, z) ~ p``: the generator runs with
        nothing observed, the values of its nodes are detached, those named in ``observed_names`` are handed to the variational
        net as observations and the others as the values of its latents.  Only q's parameters receive a gradient.  No kernel of
        its own: the log-probabilities are the nodes' kernels, the sum and the mean torch's.

        ``n_samples``: for the duration of the call the ``n_samples`` attribute of both nets (where they have one) is set to
        this, so that the dream has that many particles (None: no particle axis)."""
        observed_names = list(observed_names)
        nets = [n for n in (self.generator, self.variational) if hasattr(n, 'n_samples')]
        saved = [n.n_samples for n in nets]
        for n in nets:
            n.n_samples = n_samples
        try:
            with torch.no_grad():
                nodes_p = self.generator({}).nodes
                dream = dict((name, nodes_p[name].tensor.detach()) for name in nodes_p.keys())
            missing = [n for n in observed_names if n not in dream]
            if missing:
                raise ValueError("sleep_cost: the generator has no node named %s" % ", ".join(repr(n) for n in missing))
            nodes_q = self.variational(dream).nodes
            logq = _sum([nodes_q[n].log_prob() for n in nodes_q.keys()])
        finally:
            for n, s in zip(nets, saved):
                n.n_samples = s
        return -torch.mean(logq)


KLpq = InclusiveKLObjective          # upstream's name
