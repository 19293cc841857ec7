"""Model evaluation: the importance-sampled log-likelihood every IWAE / reweighted-wake-sleep paper reports.

``is_loglikelihood`` is the only estimator here.  Upstream ZhuSuan's ``zhusuan.evaluation`` also has annealed importance
sampling (``AIS``); that is out of scope of this package."""
import torch

from ..variational.elbo import draw_latents, run_variational
from ..variational.inclusive_kl import kernel_plan, torch_composition
from .. import _klpq_hip

__all__ = ['is_loglikelihood']


def is_loglikelihood(generator, variational, observed, axis=0):
    """log p(x) estimated with the particles of ``variational`` as proposals: ``log mean_k exp(log p(x, z_k) - log q(z_k | x))``
    along ``axis`` of the nets' log-probabilities, per datapoint -- a lower bound in expectation that tightens with the number
    of particles.  Runs under ``no_grad`` and returns a tensor without a graph; reparameterised and non-reparameterised
    latents are both fine.  The reduction is one launch (Q1 of include/zs_klpq.h in its bound-only mode); a layout the kernel
    does not take runs the torch composition of the same formula."""
    with torch.no_grad():
        run_variational(variational, observed)
        nodes_q = variational.nodes
        drawn = draw_latents(nodes_q)
        nodes_p = generator({**drawn, **observed}).nodes
        terms_p = [torch.as_tensor(nodes_p[n].log_prob()) for n in nodes_p.keys()]
        terms_q = [torch.as_tensor(nodes_q[n].log_prob()) for n in nodes_q.keys()]
        nd = max(t.dim() for t in terms_p + terms_q)
        if not -nd <= axis < nd:
            raise IndexError("Dimension out of range (expected to be in range of [%d, %d], but got %d)" % (-max(nd, 1), max(nd, 1) - 1, axis))
        axis = axis % nd
        plan = kernel_plan(terms_p, terms_q, axis)
        if isinstance(plan, str):
            return torch_composition(terms_p, terms_q, axis, False)[1]
        tp, tq, K, B, rest, _ = plan
        bound = _klpq_hip.forward(tp, tq, K, B, bound_only=True)[2]
        return bound.reshape(rest)
