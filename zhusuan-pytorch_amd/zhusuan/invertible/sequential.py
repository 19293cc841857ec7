"""``RevSequential``.  Interface and semantics of zhusuan/invertible/sequential.py:8-39 of the reference."""
import torch

from .base import RevNet

__all__ = ["RevSequential"]


class RevSequential(RevNet):
    """A list of ``RevNet`` layers applied first to last (``reverse=False``) or last to first with ``reverse=True``.
    ``None`` log-dets are skipped; when no layer reports one the log-det is ``torch.zeros([])``.

    :param layers: a list of RevNet instances.
    """

    def __init__(self, layers):
        super(RevSequential, self).__init__()
        for flow in layers:
            assert isinstance(flow, RevNet)
        self.layers = torch.nn.ModuleList(layers)

    def _walk(self, x, reverse, kwargs):
        """``x`` through every layer in the direction asked for; the log-dets that the layers report (``None`` = none) added up."""
        total = None
        for flow in (reversed(self.layers) if reverse else self.layers):
            x, log_det = flow(x, reverse=reverse, **kwargs)
            if log_det is not None:
                total = log_det if total is None else total + log_det
        return x, torch.zeros([]) if total is None else total

    def _forward(self, x, **kwargs):
        return self._walk(x, False, kwargs)

    def _inverse(self, y, **kwargs):
        return self._walk(y, True, kwargs)
