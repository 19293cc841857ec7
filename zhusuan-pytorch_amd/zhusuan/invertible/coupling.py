"""Additive coupling layers.  Interface of zhusuan/invertible/coupling.py:8-147 of the reference.  The inner networks stay
torch modules (their GEMMs are the caller's); the split before them and the merge after them are one launch each
(``zs_flow_split`` / ``zs_flow_merge``), and so are their backwards."""
import torch
import torch.nn as nn

from .base import RevNet
from .sequential import RevSequential  # noqa: F401  (coupling.py:5 of the reference exports it from here too)
from . import _functions as F

# what `from zhusuan.invertible.coupling import *` hands out in the reference as well (coupling.py:1-5 imports them by name)
__all__ = ["RevNet", "RevSequential", "get_coupling_mask", "MaskCoupling", "Coupling"]


def get_coupling_mask(n_dim, n_channel, n_mask, split_type="OddEven", dtype=torch.float32):
    """``n_mask`` masks of length ``n_dim`` for a stack of ``MaskCoupling`` layers: the first one by ``split_type``, then it
    and its complement in turn, so that consecutive layers transform complementary halves.

    "OddEven": 0, 1, 0, 1, ... (``dtype``); "Half": zeros on the first ``n_dim // 2`` positions, ones after (float32);
    "RandomHalf": one ``torch.randint(0, 2)`` draw (``dtype``).  Host tensors.  Any other ``split_type`` gives an empty list, and
    more than one channel is not implemented, both as in the reference."""
    if n_channel != 1:
        raise NotImplementedError()
    position = torch.arange(n_dim)
    if split_type == "OddEven":
        first = (position % 2).to(dtype)
    elif split_type == "Half":
        first = (position >= n_dim // 2).float()
    elif split_type == "RandomHalf":
        first = torch.randint(0, 2, (n_dim,), dtype=dtype)
    else:
        return []
    return [first if i % 2 == 0 else 1. - first for i in range(n_mask)]


def _dense_relu(n_in, n_out):
    return [nn.Linear(n_in, n_out), nn.ReLU()]


class MaskCoupling(RevNet):
    """``y = mask*x + ((1 - mask)*x + nn(mask*x)*(1 - mask))``; returns ``(y, None)``.

    ``mask`` stays a plain attribute as in the reference (not a buffer: it is not in the ``state_dict``); it is moved to
    the input's device and dtype on use, and is not differentiated.

    :param in_out_dim: input/output dimensions.
    :param mid_dim: number of units in a hidden layer.
    :param hidden: number of hidden layers.
    :param mask: a ``[in_out_dim]`` float tensor, e.g. from :func:`get_coupling_mask`.
    :param inner_nn: a module to use instead of the default MLP.
    """

    def __init__(self, in_out_dim=-1, mid_dim=-1, hidden=-1, mask=None, inner_nn=None):
        super(MaskCoupling, self).__init__()
        if inner_nn is not None:
            self.nn = inner_nn
        else:
            # an MLP in_out_dim -> mid_dim (x hidden) -> in_out_dim with ReLUs in between: linear layers at nn.0, nn.2, ...
            widths = [in_out_dim] + [mid_dim] * hidden
            body = [m for a, b in zip(widths, widths[1:]) for m in _dense_relu(a, b)]
            self.nn = nn.Sequential(*body, nn.Linear(mid_dim, in_out_dim))
        self.mask = mask

    def _couple(self, x, sign):
        x = F.prepare(x)
        mask = F.like(self.mask, x)
        if mask.numel() != x.shape[1]:
            raise RuntimeError("MaskCoupling: mask of %d elements for an input of width %d" % (mask.numel(), x.shape[1]))
        shift = self.nn(F.Split.apply(x, mask, F.MASK, 0))
        if tuple(shift.shape) != tuple(x.shape) or shift.dtype != x.dtype:
            raise RuntimeError("MaskCoupling: the inner network returned %s %s for an input %s %s"
                               % (tuple(shift.shape), shift.dtype, tuple(x.shape), x.dtype))
        return F.Merge.apply(x, mask, shift.contiguous(), sign, F.MASK, 0), None

    def _forward(self, x, **kwargs):
        return self._couple(x, 1.0)

    def _inverse(self, y, **kwargs):
        return self._couple(y, -1.0)


class Coupling(RevNet):
    """NICE's interleaved additive coupling (coupling.py:78-147): the columns are taken in pairs; one of each pair goes
    through the network and is passed on unchanged, the other is shifted by the network's output.  An odd width raises
    ``RuntimeError`` (the reference's ``reshape`` fails).  Returns ``(y, None)``.

    :param in_out_dim: input/output dimensions.
    :param mid_dim: number of units in a hidden layer.
    :param hidden: number of hidden layers.
    :param mask_config: 1 if transform odd units, 0 if transform even units.
    """

    def __init__(self, in_out_dim, mid_dim, hidden, mask_config):
        super(Coupling, self).__init__()
        half = in_out_dim // 2
        self.mask_config = mask_config
        # half -> mid_dim (in_block), hidden - 1 blocks mid_dim -> mid_dim (mid_block), mid_dim -> half (out_block)
        self.in_block = nn.Sequential(*_dense_relu(half, mid_dim))
        self.mid_block = nn.ModuleList(nn.Sequential(*_dense_relu(mid_dim, mid_dim)) for _ in range(hidden - 1))
        self.out_block = nn.Linear(mid_dim, half)

    def _couple(self, x, sign):
        x = F.prepare(x)
        B, W = x.shape
        if W % 2:
            raise RuntimeError("shape '[%d, %d, 2]' is invalid for input of size %d" % (B, W // 2, B * W))
        # coupling.py:112-115: mask_config set -> on = x[:, :, 0], off = x[:, :, 1]; `off` feeds the network
        sel = 1 if self.mask_config else 0
        h = self.in_block(F.Split.apply(x, None, F.INTERLEAVE, sel))
        for block in self.mid_block:
            h = block(h)
        shift = self.out_block(h)
        return F.Merge.apply(x, None, shift.contiguous(), sign, F.INTERLEAVE, sel), None

    def _forward(self, x, **kwargs):
        return self._couple(x, 1.0)

    def _inverse(self, x, **kwargs):
        return self._couple(x, -1.0)
