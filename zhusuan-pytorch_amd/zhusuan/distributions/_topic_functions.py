"""The autograd Function of AdmixtureMultinomial over the kernels of include/zs_topic.h (``zhusuan._topic_hip``, imported at call
time: ``import zhusuan`` loads neither that module nor its library).  ``H`` is the contiguous ``[R, K]`` view of the document
logits, ``B`` the ``[K, V]`` topic logits, ``X`` the ``[Dx, V]`` counts with ``R % Dx == 0``."""
import torch
from torch.autograd.function import once_differentiable

MAX_TOPICS = 128          # zs_topic_max_topics(), restated so that routing does not import the binding; checked when the library loads


class AdmixtureLogProb(torch.autograd.Function):
    """``lp [R]``.  The forward keeps the small ``prep`` workspace (lse, N, Z, log Z, E) instead of anything of size ``[R, V]``;
    the backward launches the ``dH`` kernels only if ``H`` needs a gradient and the ``dB`` kernels only if ``B`` does.
    ``record`` (a dict of the caller's, may be None) receives ``needs_input_grad`` and the number of elements of the partial
    workspace each gradient allocated (None for one that did not run); the workspaces themselves are released."""

    @staticmethod
    def forward(ctx, H, B, X, record):
        from .. import _topic_hip
        lp, prep = _topic_hip.logprob(H, B, X)
        ctx.save_for_backward(H, B, X, prep)
        ctx.record = record
        ctx.mark_non_differentiable(prep)
        ctx.set_materialize_grads(False)
        return lp, prep

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gprep):
        from .. import _topic_hip
        H, B, X, prep = ctx.saved_tensors
        want_h, want_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dH = dB = part_h = part_b = None
        if g is not None:
            g = g.contiguous()
            if want_h:
                dH, part_h = _topic_hip.grad_doc(H, B, X, g, prep)
            if want_b:
                dB, part_b = _topic_hip.grad_topic(H, B, X, g, prep)
        if ctx.record is not None:
            ctx.record.update(needs_input_grad=(bool(want_h), bool(want_b)),
                              grad_doc_workspace_elems=None if part_h is None else part_h.numel(),
                              grad_topic_workspace_elems=None if part_b is None else part_b.numel())
        return dH, dB, None, None


def torch_log_prob(H, B, X):
    """The torch composition: ``sum_v X log(softmax(H) @ softmax(B))`` with ``0 log 0 = 0``; ``X`` broadcasts against the rows.
    The column shift of the kernels (``c_v = max_k log phi[k, v]``, which cancels and so carries no gradient) keeps a word that
    is rare under every topic finite in float32."""
    log_phi = torch.log_softmax(B, -1)
    c = log_phi.max(0).values.detach()
    log_pred = c + torch.log(torch.softmax(H, -1) @ torch.exp(log_phi - c))
    return (X * torch.where(X > 0, log_pred, torch.zeros_like(log_pred))).sum(-1)
