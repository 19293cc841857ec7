"""``RevNet``: base class of the invertible layers.  Interface of zhusuan/invertible/base.py:10-31 of the reference."""
import torch.nn as nn

__all__ = ["RevNet"]


class RevNet(nn.Module):
    """A reversible network: subclasses implement ``_forward`` and ``_inverse``, both returning ``(y, log_det_J)``."""

    def _forward(self, *inputs, **kwargs):
        raise NotImplementedError()

    def _inverse(self, *inputs, **kwargs):
        raise NotImplementedError()

    def forward(self, *inputs, reverse=False, **kwargs):
        """``reverse=False`` runs ``_forward``, ``reverse=True`` runs ``_inverse`` (base.py:23-31)."""
        if not reverse:
            return self._forward(*inputs, **kwargs)
        return self._inverse(*inputs, **kwargs)
