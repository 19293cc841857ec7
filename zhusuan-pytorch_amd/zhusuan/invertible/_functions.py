"""``torch.autograd.Function``s of the flow layers: each forward and each backward is ONE launch of a kernel of
include/zs_flow.h, reached through the module-level functions of ``zhusuan._flow_hip`` (looked up at call time)."""
import torch

from .. import _flow_hip

MASK, INTERLEAVE = 0, 1


def prepare(x, name="input"):
    """The host layer's input rule: float32 / float64, made contiguous; anything else raises naming the dtype."""
    if not isinstance(x, torch.Tensor):
        raise RuntimeError("zhusuan.invertible: %s must be a tensor, got %s" % (name, type(x).__name__))
    if x.dtype not in (torch.float32, torch.float64):
        raise RuntimeError("zhusuan.invertible: %s must be float32 or float64, got %s" % (name, x.dtype))
    if x.dim() != 2:
        raise RuntimeError("zhusuan.invertible: %s must be [batch, dim], got shape %s" % (name, tuple(x.shape)))
    return x if x.is_contiguous() else x.contiguous()


def like(mask, x):
    """A [D] operand (mask, parameter) in x's dtype, on x's device, contiguous."""
    m = mask.detach() if mask.requires_grad else mask
    if m.dtype != x.dtype or m.device != x.device:
        m = m.to(device=x.device, dtype=x.dtype)
    return m.reshape(-1).contiguous()


class Split(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask, mode, sel):
        B, D = x.shape
        out = x.new_empty((B, D) if mode == MASK else (B, D // 2))
        _flow_hip.split(mode, x, mask, out, sel)
        ctx.mode, ctx.sel, ctx.shape = mode, sel, (B, D)
        ctx.mask = mask
        return out

    @staticmethod
    def backward(ctx, g):
        g = g.contiguous()
        gx = g.new_empty(ctx.shape)
        _flow_hip.split_bwd(ctx.mode, g, ctx.mask, gx, ctx.sel)
        return gx, None, None, None


class Merge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask, shift, sign, mode, sel):
        y = torch.empty_like(x)
        _flow_hip.merge(mode, x, mask, shift, sign, y, sel)
        ctx.mode, ctx.sel, ctx.sign, ctx.mask = mode, sel, sign, mask
        ctx.shift_shape = tuple(shift.shape)
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = gy.contiguous()
        gx = torch.empty_like(gy)
        gshift = gy.new_empty(ctx.shift_shape)
        _flow_hip.merge_bwd(ctx.mode, gy, ctx.mask, ctx.sign, gx, gshift, ctx.sel)
        return gx, None, gshift, None, None, None


class Scale(torch.autograd.Function):
    """In place like scaling.py:28: the returned tensor IS the input (``mark_dirty``); the backward reads the saved OUTPUT."""

    @staticmethod
    def forward(ctx, x, log_scale, sign):
        ls = like(log_scale, x)
        logdet = x.new_empty(())
        _flow_hip.scale_fwd(x, ls, sign, x, logdet)
        ctx.mark_dirty(x)
        ctx.sign = sign
        ctx.ls_shape, ctx.ls_dtype = tuple(log_scale.shape), log_scale.dtype
        ctx.save_for_backward(x, ls)
        return x, logdet

    @staticmethod
    def backward(ctx, gy, g_logdet):
        y, ls = ctx.saved_tensors
        gy = torch.zeros_like(y) if gy is None else gy.contiguous()
        gx = torch.empty_like(gy)
        g_ls = torch.empty_like(ls)
        gl = None if g_logdet is None else g_logdet.contiguous()
        _flow_hip.scale_bwd(gy, y, ls, gl, ctx.sign, gx, g_ls)
        return gx, g_ls.reshape(ctx.ls_shape).to(ctx.ls_dtype), None


class MadeAffine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, net):
        u = torch.empty_like(x)
        logdet = torch.empty_like(x)
        _flow_hip.made_fwd(x, net, u, logdet)
        ctx.save_for_backward(x, net)
        return u, logdet

    @staticmethod
    def backward(ctx, gu, gld):
        x, net = ctx.saved_tensors
        if gu is None and gld is None:
            return None, None
        gu = None if gu is None else gu.contiguous()
        gld = None if gld is None else gld.contiguous()
        gx = torch.empty_like(x)
        gnet = torch.empty_like(net)
        _flow_hip.made_bwd(gu, gld, x, net, gx, gnet)
        return gx, gnet


class Tail(torch.autograd.Function):
    """FlowDistribution's log-density of the base, row sum and log-det add (flow_distribution.py:49-51)."""

    @staticmethod
    def forward(ctx, z, loc, scale, logdet, base, param_rows, logdet_kind):
        out = z.new_empty((z.shape[0],))
        _flow_hip.tail(base, z, loc, scale, param_rows, logdet, logdet_kind, out)
        ctx.base, ctx.param_rows, ctx.logdet_kind = base, param_rows, logdet_kind
        ctx.logdet_shape = None if logdet is None else tuple(logdet.shape)
        ctx.save_for_backward(z, loc, scale)
        return out

    @staticmethod
    def backward(ctx, g):
        z, loc, scale = ctx.saved_tensors
        g = g.contiguous()
        gz = torch.empty_like(z)
        rows = ctx.logdet_kind == _flow_hip.LOGDET_ROWS and ctx.needs_input_grad[3]
        gl = g.new_empty((z.shape[0],)) if rows else None
        _flow_hip.tail_bwd(ctx.base, g, z, loc, scale, ctx.param_rows, gz, gl)
        if ctx.logdet_kind == _flow_hip.LOGDET_SCALAR and ctx.needs_input_grad[3]:
            gl = g.sum()
        if gl is not None:
            gl = gl.reshape(ctx.logdet_shape)
        return gz, None, None, gl, None, None, None
