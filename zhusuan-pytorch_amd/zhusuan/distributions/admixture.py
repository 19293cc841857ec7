"""AdmixtureMultinomial: the likelihood of the logistic-normal topic model (the reference's unfinished
``examples/topic_models/lntm_mcem.py`` and its tutorial): bag-of-words counts under ``softmax(doc_logits) @ softmax(topic_logits)``,

    log_prob(x) = sum_v x_v log( sum_k softmax(doc_logits)_k softmax(topic_logits[k])_v ),

upstream's ``UnnormalizedMultinomial(log(theta @ phi), normalize_logits=False)`` -- no multinomial coefficient -- without the
``[rows, V]`` logits ever being formed.  Up to 128 topics, on a HIP device, the value and both gradients come from the fused
matrix-core kernels of include/zs_topic.h; more topics, or CPU tensors, run the torch composition; ``last_path`` /
``zhusuan.explain`` say which.  What the kernel path saves is memory: nothing of size ``[rows, V]`` is allocated or kept for the
backward.  In time it is ahead of the torch composition at about 100 rows and currently behind it at about 1000 (0.62 - 0.78 x at
K = 50, V = 12 419)."""
import torch

from .base import Distribution
from .categorical import _numel, sum_trailing
from .utils import assert_same_log_float_dtype
from . import _topic_functions as _F
from .. import _hip
from ..utils import note_path

__all__ = ['AdmixtureMultinomial']

NO_SAMPLE = ("AdmixtureMultinomial%s cannot be sampled: the total count of a draw is not a parameter of the distribution "
             "(as with upstream's UnnormalizedMultinomial); observe the node")


class AdmixtureMultinomial(Distribution):
    """
    :param doc_logits: float tensor ``[..., K]``: the unnormalised log-proportions of the K topics, one row per document (and
        chain).  A row may spread up to 60 nats on the kernel path (include/zs_topic.h states the domain).
    :param topic_logits: float tensor ``[K, V]``: the unnormalised log-probabilities of the V words under each topic.
    ``batch_shape`` is ``doc_logits.shape[:-1]`` and an event is a vector of V non-negative counts.  ``log_prob(x)`` takes ``x`` of
    the full shape ``batch_shape + [V]`` or of ``batch_shape[-j:] + [V]``, shared over the leading axes (one count matrix for all
    chains, never expanded).  There is no gradient with respect to ``x``.
    """
    _event_ndims = 1

    def __init__(self, doc_logits, topic_logits, dtype=None, group_ndims=0, device=None, **kwargs):
        device = _hip.resolve_device(device, doc_logits, topic_logits)
        self._doc_logits = torch.as_tensor(doc_logits, dtype=dtype).to(device)
        self._topic_logits = torch.as_tensor(topic_logits, dtype=dtype).to(device)
        dtype = assert_same_log_float_dtype([(self._doc_logits, 'AdmixtureMultinomial.doc_logits'),
                                             (self._topic_logits, 'AdmixtureMultinomial.topic_logits')])
        if self._doc_logits.dim() < 1 or self._doc_logits.shape[-1] < 1:
            raise ValueError("doc_logits must have a last axis of at least one topic, got shape %s" % (tuple(self._doc_logits.shape),))
        K = int(self._doc_logits.shape[-1])
        if self._topic_logits.dim() != 2 or self._topic_logits.shape[0] != K or self._topic_logits.shape[1] < 1:
            raise ValueError("topic_logits must have shape [%d, V] (the last axis of doc_logits %s has %d topics), got %s"
                             % (K, tuple(self._doc_logits.shape), K, tuple(self._topic_logits.shape)))
        self._n_topics, self._n_words = K, int(self._topic_logits.shape[1])
        super(AdmixtureMultinomial, self).__init__(dtype=dtype, is_continuous=False, is_reparameterized=False,
                                                   group_ndims=group_ndims, device=device, **kwargs)
        self.last_path = None          # which path the last log_prob ran on (zhusuan.explain)
        self.last_workspaces = {}      # filled by the kernel path's backward: which gradient launches ran, the sizes of their partials

    @property
    def doc_logits(self):
        return self._doc_logits

    @property
    def topic_logits(self):
        return self._topic_logits

    @property
    def n_topics(self):
        return self._n_topics

    @property
    def n_words(self):
        return self._n_words

    def _batch_shape(self):
        return self._doc_logits.shape[:-1]

    def _sample(self, n_samples=1, **kwargs):
        raise NotImplementedError(NO_SAMPLE % "")

    def _log_prob_sum(self, given=None, n_fold=0):
        given = self.sample_cache if given is None else given          # (an observed node primes sample_cache)
        if given is None:
            raise RuntimeError("AdmixtureMultinomial.log_prob(None): there is no observed value, and the distribution cannot be sampled")
        x = torch.as_tensor(given, dtype=self._dtype).to(self._doc_logits.device)
        batch, K, V = tuple(self._batch_shape()), self._n_topics, self._n_words
        lead = tuple(x.shape[:-1])
        if x.dim() < 1 or x.shape[-1] != V or len(lead) > len(batch) or lead != batch[len(batch) - len(lead):]:
            raise ValueError("the value must have shape batch_shape[-j:] + [V] for some j, with batch_shape %s and V = %d; got %s"
                             % (batch, V, tuple(x.shape)))
        R, Dx = _numel(batch), _numel(lead)
        H, B = self._doc_logits, self._topic_logits
        why = None
        if H.device.type != "cuda":
            why = "the operands are on the CPU"
        elif K > _F.MAX_TOPICS:
            why = "more than %d topics are outside the fused kernels' domain (zs_topic_max_topics)" % _F.MAX_TOPICS
        elif R == 0:
            why = "there are no rows"
        if why is not None:
            lp = _F.torch_log_prob(H, B, x)
            note_path(self, "torch composition (softmax, matmul, log, row sum)", why)
            return sum_trailing(lp, n_fold)
        self.last_workspaces = {}
        lp, _ = _F.AdmixtureLogProb.apply(H.reshape(R, K).contiguous(), B.contiguous(), x.detach().reshape(Dx, V).contiguous(),
                                          self.last_workspaces)
        note_path(self, "zs_topic_prepare + zs_topic_logprob: the product tile by tile in matrix-core accumulators; "
                        "zs_topic_grad_doc / zs_topic_grad_topic backward")
        return sum_trailing(lp.reshape(batch), n_fold)
