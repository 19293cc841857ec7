"""``zhusuan.transform``: flows that are not ``RevNet``s (upstream ZhuSuan's ``zs.transform``; a planar map has no closed-form
inverse).  ``PlanarFlow`` (Rezende & Mohamed 2015) and ``HouseholderFlow`` (Tomczak & Welling 2016) apply their whole stack of
layers in one launch of the kernels of include/zs_nf.h, up to 64 dimensions; wider rows run the torch composition of the same
formulas on the device, and ``last_path`` / ``zhusuan.explain`` say which ran and why.  Both have the calling convention of
``ELBO(transform=)``: with ``name='z'``,

    ELBO(gen, var, transform=zs.transform.PlanarFlow(40, 8, name='z'), transform_var=['z'])
"""
import torch
import torch.nn as nn

from . import _functions as _F
from .. import _nf_hip
from ..utils import note_path

__all__ = ['PlanarFlow', 'HouseholderFlow']

WIDE = "rows wider than %d: the kernels of include/zs_nf.h keep a row in one wave" % _nf_hip.MAX_DIM


def _check(z_dim, n_flows):
    if int(z_dim) < 1:
        raise ValueError("z_dim must be at least 1, got %r" % (z_dim,))
    if int(n_flows) < 1:
        raise ValueError("n_flows must be at least 1, got %r" % (n_flows,))


def _launches(L):
    return -(-L // _nf_hip.MAX_LAYERS)


class _Flow(nn.Module):
    def _result(self, z_out, log_det):
        return ({self.name: z_out} if self.name is not None else z_out), log_det


class PlanarFlow(_Flow):
    """``n_flows`` planar layers ``z <- z + uh_l tanh(w_l.z + b_l)``; ``uh_l`` is ``u_l`` with its component along ``w_l`` moved so
    that ``w_l.uh_l = softplus(w_l.u_l) - 1 > -1``, which keeps every layer invertible.

    ``forward(z)`` takes a ``[B, z_dim]`` tensor, or a tuple whose first element is one (how ``ELBO`` calls a transform), and
    returns ``(z_out, log_det)`` with ``log_det [B, 1]`` the SUM over the layers -- ``({name: z_out}, log_det)`` when ``name``
    is given.  Parameters: ``u``, ``w`` ``[n_flows, z_dim]`` and ``b`` ``[n_flows]``, drawn layer by layer in the order
    ``u_l, w_l, b_l`` from ``torch.rand``."""

    def __init__(self, z_dim, n_flows=1, name=None):
        super(PlanarFlow, self).__init__()
        _check(z_dim, n_flows)
        self.z_dim, self.n_flows, self.name = int(z_dim), int(n_flows), name
        drawn = [[torch.rand(shape) for shape in ([1, self.z_dim], [1, self.z_dim], [1])] for _ in range(self.n_flows)]
        self.u = nn.Parameter(torch.cat([d[0] for d in drawn], 0))
        self.w = nn.Parameter(torch.cat([d[1] for d in drawn], 0))
        self.b = nn.Parameter(torch.cat([d[2] for d in drawn], 0))
        self.last_path = None          # which kernels the last forward ran on (zhusuan.explain)

    def forward(self, z, **kwargs):
        if isinstance(z, (tuple, list)):
            z = z[0]
        if z.dim() != 2 or z.shape[1] != self.z_dim:
            raise ValueError("PlanarFlow(%d): expected a [B, %d] tensor, got %s" % (self.z_dim, self.z_dim, tuple(z.shape)))
        u, w, b = (p.to(z.dtype) for p in (self.u, self.w, self.b))
        if self.z_dim > _nf_hip.MAX_DIM:
            z_out, log_det = _F.planar_torch(z, u, w, b)
            note_path(self, "torch composition (matmul, tanh, log per layer)", WIDE)
        else:
            z_out, log_det = _F.PlanarStack.apply(z.contiguous(), u.contiguous(), w.contiguous(), b.contiguous())
            note_path(self, "P1 zs_nf_planar_fwd: %d layers in %d launch(es)" % (self.n_flows, _launches(self.n_flows)))
        return self._result(z_out, log_det[:, None])


class HouseholderFlow(_Flow):
    """``n_flows`` Householder reflections ``z <- z - 2 v_l (v_l.z) / |v_l|^2``.  The vectors come from a chain of linear layers
    that never reads ``z``: ``v_1 = v_layers[0](aux)``, ``v_l = v_layers[l-1](v_{l-1})``; they are computed first and the
    reflections applied in one launch.  A reflection preserves volume: the log-det is ``zeros([1, 1])``.

    ``forward((z, aux))`` returns ``(z_out, log_det)``, or ``({name: z_out}, log_det)`` when ``name`` is given."""

    def __init__(self, z_dim, v_dim, n_flows, name=None):
        super(HouseholderFlow, self).__init__()
        _check(z_dim, n_flows)
        self.z_dim, self.v_dim, self.n_flows, self.name = int(z_dim), int(v_dim), int(n_flows), name
        self.v_layers = nn.ModuleList([nn.Linear(self.v_dim if l == 0 else self.z_dim, self.z_dim) for l in range(self.n_flows)])
        self.last_path = None          # which kernels the last forward ran on (zhusuan.explain)

    def forward(self, inputs, **kwargs):
        z, v = inputs[0], inputs[1]
        if z.dim() != 2 or z.shape[1] != self.z_dim:
            raise ValueError("HouseholderFlow(%d): expected a [B, %d] tensor, got %s" % (self.z_dim, self.z_dim, tuple(z.shape)))
        vs = []
        for layer in self.v_layers:
            v = layer(v)
            vs.append(v)
        vs = torch.stack(vs, 0).to(z.dtype)
        if self.z_dim > _nf_hip.MAX_DIM:
            z_out = _F.householder_torch(z, vs)
            note_path(self, "torch composition (two row sums and an axpy per layer)", WIDE)
        else:
            z_out = _F.HouseholderStack.apply(z.contiguous(), vs)
            note_path(self, "H1 zs_nf_householder_fwd: %d reflections in %d launch(es)" % (self.n_flows, _launches(self.n_flows)))
        return self._result(z_out, torch.zeros([1, 1], device=z.device))
