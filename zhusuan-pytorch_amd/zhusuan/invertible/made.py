"""MADE / MAF building blocks.  Interface of zhusuan/invertible/made.py:9-122 of the reference; the affine after the masked
network is one launch each way (``zs_flow_made_fwd`` / ``zs_flow_made_bwd``) on the network's ``[B, 2D]`` output read in
place, and one column of the inverse is one launch (``zs_flow_made_inv_col``)."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as TF

from .base import RevNet
from . import _functions as F
from .. import _flow_hip

__all__ = ["RevNet", "MaskedLinear", "MADE"]


class MaskedLinear(nn.Linear):
    """MADE building block layer: a linear layer whose weight is multiplied by a fixed 0 / 1 mask (buffer ``mask``); with
    ``cond_label_size`` a second, unmasked weight ``cond_weight`` maps a conditioning label onto the outputs."""

    def __init__(self, input_size, n_outputs, mask, cond_label_size=None):
        nn.Linear.__init__(self, input_size, n_outputs)
        self.cond_label_size = cond_label_size
        self.register_buffer("mask", mask)
        if cond_label_size is None:
            return
        # U(0, 1) / sqrt(fan-in), drawn after the linear layer's own initialisation (the reference's draw order)
        draw = torch.rand(n_outputs, cond_label_size)
        self.cond_weight = nn.Parameter(draw.div_(math.sqrt(cond_label_size)))

    def forward(self, x, cond_y=None, masked_weight=None):
        """``masked_weight``: ``weight * mask`` computed by the caller (MADE's inverse forms it once per call)."""
        w = self.weight * self.mask if masked_weight is None else masked_weight
        out = TF.linear(x, w, self.bias)
        if cond_y is not None:
            out = out + TF.linear(cond_y, self.cond_weight)
        return out


_ACTIVATIONS = {"relu": nn.ReLU, "tanh": nn.Tanh}


class MADE(RevNet):
    """
    :param input_size: a scalar; dim of inputs
    :param hidden_size: a scalar; dim of hidden layers
    :param n_hidden: a scalar; number of hidden layers
    :param cond_label_size: size of the conditioning label, or None
    :param input_order: a str; variable order for creating the autoregressive masks (sequential|random)
    :param input_degrees: degrees provided by the user (the order flipped from the previous layer in a stack of MADEs)
    :param activation: a str; 'relu' or 'tanh'
    """

    def __init__(self, input_size, hidden_size, n_hidden, cond_label_size=None,
                 input_order="sequential", input_degrees=None, activation="relu"):
        super(MADE, self).__init__()
        for name, fill in (("base_dist_mean", 0.0), ("base_dist_var", 1.0)):
            self.register_buffer(name, torch.full((input_size,), fill))
        masks, self.input_degrees = self.create_mask(input_size, hidden_size, n_hidden, input_order, input_degrees)
        if activation not in _ACTIVATIONS:
            raise ValueError("Invalid activation function")
        act = _ACTIVATIONS[activation]()
        # masks[0] feeds `net_input`; every later mask is one (activation, MaskedLinear) pair of `net`, so that the linear layers
        # sit at net.1, net.3, ...; the last one emits m and loga side by side: its mask is the output mask twice
        self.net_input = MaskedLinear(input_size, hidden_size, masks[0], cond_label_size)
        rest = masks[1:-1] + [torch.cat([masks[-1], masks[-1]], dim=0)]
        pairs = []
        for m in rest:
            pairs.extend([act, MaskedLinear(hidden_size, m.shape[0], m)])
        self.net = nn.Sequential(*pairs)

    @staticmethod
    def create_mask(input_size, hidden_size, n_hidden, input_order='sequential', input_degrees=None):
        """Masks of MADE / MAF (Germain et al. 2015, section 4, https://arxiv.org/abs/1502.03509): every unit gets a degree, and
        a unit of one layer may read a unit of the layer below only if its own degree is at least that unit's.  Inputs carry
        degrees 0 .. D-1 (their order, or ``input_degrees``), hidden units cycle through 0 .. D-2 ('sequential') or are drawn
        ('random'), outputs carry the degree of their input minus one, which makes output i blind to input i.

        Returns: the list of ``n_hidden + 2`` float masks ``[units above, units below]`` and the input degrees.  With
        'random' the draws are made in the reference's order (inputs, each hidden layer, outputs), so a seed gives its masks."""
        D = input_size
        given = input_degrees is not None
        if input_order == "sequential":
            layers = [input_degrees if given else torch.arange(D)]
            layers += [torch.arange(hidden_size) % (D - 1) for _ in range(n_hidden + 1)]
            layers.append((input_degrees if given else torch.arange(D)) % D - 1)
        elif input_order == "random":
            layers = [input_degrees if given else torch.randperm(D)]
            for _ in range(n_hidden + 1):
                lowest = min(int(layers[-1].min()), D - 1)
                layers.append(torch.randint(lowest, D, (hidden_size,)))
            lowest = min(int(layers[-1].min()), D - 1)
            layers.append(input_degrees - 1 if given else torch.randint(lowest, D, (D,)) - 1)
        else:
            raise NotImplementedError("input_order must be in 'sequential' or 'random'")
        masks = [(above[:, None] >= below[None, :]).float() for below, above in zip(layers, layers[1:])]
        return masks, layers[0]

    def _masked_weights(self):
        layers = [self.net_input] + [m for m in self.net if isinstance(m, MaskedLinear)]
        return {id(m): m.weight * m.mask for m in layers}

    def _run_net(self, x, cond_y, weights=None):
        """The masked network's ``[B, 2D]`` output; ``weights``: masked weights formed once by the caller."""
        if weights is None:
            return self.net(self.net_input(x, cond_y))
        h = self.net_input(x, cond_y, masked_weight=weights[id(self.net_input)])
        for m in self.net:
            h = m(h, masked_weight=weights[id(m)]) if isinstance(m, MaskedLinear) else m(h)
        return h

    def _forward(self, x, cond_y=None, **kwargs):
        """MAF eq. 4-5: ``u = (x - m) * exp(-loga)`` and the ``[B, D]`` log-det ``-loga`` (made.py:106-112)."""
        x = F.prepare(x)
        net = self._run_net(x, cond_y)
        return F.MadeAffine.apply(x, net.contiguous())

    def _inverse(self, u, cond_y=None, **kwargs):
        """made.py:114-122: the columns are filled in ``input_degrees`` order, one pass of the network per column; returns
        ``(x, loga)``.  ``weight * mask`` of every layer is formed once per call instead of once per pass (same values).

        When grad mode is off, or neither ``u``, ``cond_y`` nor a parameter requires grad, a column is one launch of the
        column kernel; otherwise the reference's own op sequence runs, so that autograd sees what it sees there."""
        u = F.prepare(u)
        weights = self._masked_weights()
        needs_grad = torch.is_grad_enabled() and (
            u.requires_grad or (cond_y is not None and cond_y.requires_grad) or any(p.requires_grad for p in self.parameters()))
        x = torch.zeros_like(u)
        loga = None
        for i in self.input_degrees:
            net = self._run_net(x, cond_y, weights)
            if needs_grad:
                m, loga = net.chunk(chunks=2, dim=1)
                x[:, i] = u[:, i] * torch.exp(loga[:, i]) + m[:, i]
            else:
                net = net.contiguous()
                _flow_hip.made_inv_col(u, net, x, int(i))
                loga = net[:, net.shape[1] // 2:]
        return x, loga
