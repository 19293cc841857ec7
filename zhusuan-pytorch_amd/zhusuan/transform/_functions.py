"""Autograd Functions of the planar and Householder flow stacks over the kernels of include/zs_nf.h (``zhusuan._nf_hip``, looked
up at call time).  Rows are the contiguous ``[R, D]`` view; a stack deeper than ``_nf_hip.MAX_LAYERS`` runs as consecutive chunks
of at most that many layers.  What is saved for the backward is the input of every chunk and the parameters: the backward
kernels recompute the layers."""
import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from .. import _nf_hip


def _chunks(L):
    step = _nf_hip.MAX_LAYERS
    return [(c, min(c + step, L)) for c in range(0, L, step)]


class PlanarStack(torch.autograd.Function):
    """P1: ``(y [R, D], logdet [R])`` of ``L`` planar layers ``u, w [L, D]``, ``b [L]``: one launch per chunk forward; backward
    one launch per chunk for the row cotangent and the per-workgroup partial sums, plus P1f when a parameter requires grad."""

    @staticmethod
    def forward(ctx, z, u, w, b):
        ctx.set_materialize_grads(False)          # an output that did not enter the loss brings None, not zeros
        xs, logdet = [], None
        for c0, c1 in _chunks(u.shape[0]):
            xs.append(z)
            z, ld = _nf_hip.planar_fwd(u[c0:c1], w[c0:c1], b[c0:c1], z)
            logdet = ld if logdet is None else logdet + ld          # in chunk order
        ctx.save_for_backward(u, w, b, *xs)
        return z, logdet

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, gld):
        u, w, b = ctx.saved_tensors[:3]
        xs = ctx.saved_tensors[3:]
        wz, wu, ww, wb = ctx.needs_input_grad
        wp = wu or ww or wb
        if (gy is None and gld is None) or not (wz or wp):
            return None, None, None, None
        g = None if gy is None else gy.contiguous()
        gld = None if gld is None else gld.contiguous()          # shared by every chunk
        spans = _chunks(u.shape[0])
        gus, gws, gbs = [], [], []
        for n in range(len(spans) - 1, -1, -1):
            c0, c1 = spans[n]
            uc, wc, bc = u[c0:c1], w[c0:c1], b[c0:c1]
            g, partials = _nf_hip.planar_bwd(uc, wc, bc, xs[n], gy=g, gld=gld, want_gx=wz or n > 0, want_partials=wp)
            if wp:
                gu, gw, gb = _nf_hip.planar_finish(uc, wc, partials, want_gu=wu, want_gw=ww, want_gb=wb)
                gus.insert(0, gu), gws.insert(0, gw), gbs.insert(0, gb)

        def whole(parts, want):
            if not want:
                return None
            return parts[0] if len(parts) == 1 else torch.cat(parts, 0)
        return (g if wz else None), whole(gus, wu), whole(gws, ww), whole(gbs, wb)


class HouseholderStack(torch.autograd.Function):
    """H1: ``y [R, D]`` after the reflections ``v [L, R, D]``: one launch per chunk each way."""

    @staticmethod
    def forward(ctx, z, v):
        ctx.set_materialize_grads(False)
        xs = []
        for c0, c1 in _chunks(v.shape[0]):
            xs.append(z)
            z = _nf_hip.householder_fwd(v[c0:c1], z)
        ctx.save_for_backward(v, *xs)
        return z

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        v = ctx.saved_tensors[0]
        xs = ctx.saved_tensors[1:]
        wz, wv = ctx.needs_input_grad
        if gy is None or not (wz or wv):
            return None, None
        g = gy.contiguous()
        spans = _chunks(v.shape[0])
        gvs = []
        for n in range(len(spans) - 1, -1, -1):
            c0, c1 = spans[n]
            g, gv = _nf_hip.householder_bwd(v[c0:c1], xs[n], g, want_gx=wz or n > 0, want_gv=wv)
            gvs.insert(0, gv)
        if not wv:
            return g, None
        return (g if wz else None), (gvs[0] if len(gvs) == 1 else torch.cat(gvs, 0))


# ---------------------------------------------------------------------------------------------------- rows wider than MAX_DIM
def planar_torch(z, u, w, b):
    """The formulas of include/zs_nf.h as a torch composition (differentiable by autograd): rows wider than the kernels take."""
    logdet = z.new_zeros(z.shape[0])
    for l in range(u.shape[0]):
        s, n = (w[l] * u[l]).sum(), (w[l] * w[l]).sum()
        uh = u[l] + (F.softplus(s) - 1. - s) * w[l] / n
        c = (w[l] * uh).sum()
        t = torch.tanh(z @ w[l] + b[l])
        z = z + uh * t[:, None]
        logdet = logdet + torch.log(torch.abs(1. + (1. - t * t) * c))
    return z, logdet


def householder_torch(z, v):
    for l in range(v.shape[0]):
        along = (v[l] * z).sum(1, keepdim=True) / (v[l] * v[l]).sum(1, keepdim=True)
        z = z - 2. * v[l] * along
    return z
