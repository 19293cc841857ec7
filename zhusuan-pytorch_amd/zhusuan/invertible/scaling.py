"""``Scaling``.  Interface and semantics of zhusuan/invertible/scaling.py:13-34 of the reference; the multiply and the
log-det are one launch (``zs_flow_scale_fwd``), the backward another (``zs_flow_scale_bwd``)."""
import torch
import torch.nn as nn

from .base import RevNet
from . import _functions as F

__all__ = ["Scaling"]


class Scaling(RevNet):
    """``y = x * exp(log_scale)`` with ``log_det_J = sum(log_scale)`` (a 0-d tensor), IN PLACE as in the reference: the
    returned tensor is the input.  A leaf tensor that requires grad therefore raises ``RuntimeError`` (autograd's rule
    for in-place operations); a non-contiguous input is copied first and the copy is returned.

    :param dim: input/output dimensions.
    """

    def __init__(self, dim):
        super(Scaling, self).__init__()
        self.log_scale = nn.Parameter(torch.zeros([1, dim]), requires_grad=True)

    def _forward(self, x, **kwargs):
        return F.Scale.apply(F.prepare(x), self.log_scale, 1.0)

    def _inverse(self, y, **kwargs):
        return F.Scale.apply(F.prepare(y), self.log_scale, -1.0)
