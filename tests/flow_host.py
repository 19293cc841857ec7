"""TEST INFRASTRUCTURE, companion of tests/host_backend.py for ``zhusuan.invertible`` and ``FlowDistribution``:
``install()`` replaces the kernel functions of the flow binding (``zhusuan._flow_hip.split`` ... ``tail_bwd``) by a torch
restatement of the contract of include/zs_flow.h on CPU tensors, so that the layers' host logic (autograd wiring, in-place
semantics, launch counts, shapes) runs on a GPU-less machine.  The package itself contains no such routing.

The restatement is written in the tensors' own dtype, one torch op per operation of the header, in the header's order (no
fused multiply-add).  ``count_launches()`` (``Router.count`` of tests/host_routing.py) wraps whatever functions are
currently installed -- the real ones on the hip back-end -- and counts their calls by name."""
import math

import torch

import host_routing

NAMES = ("split", "split_bwd", "merge", "merge_bwd", "scale_fwd", "scale_bwd", "made_fwd", "made_bwd", "made_inv_col", "tail",
         "tail_bwd")
MASK, INTERLEAVE = 0, 1
NORMAL, LOGISTIC = 0, 1
LOGDET_NONE, LOGDET_SCALAR, LOGDET_ROWS = 0, 1, 2


def _host(*tensors):
    host_routing.host_only("flow_host", tensors)
    for t in tensors:
        if t is None:
            continue
        if t.dtype not in (torch.float32, torch.float64):
            raise RuntimeError("zhusuan.invertible: tensors must be float32 or float64, got %s" % t.dtype)
        if not t.is_contiguous():
            raise RuntimeError("zhusuan.invertible: kernel operands must be contiguous")


def split(mode, x, mask, out, sel=0):
    _host(x, mask, out)
    with torch.no_grad():
        if mode == MASK:
            out.copy_(mask * x)
        else:
            if x.shape[1] % 2:
                raise RuntimeError("zs_flow_split failed with code -1: invalid argument (ZS_EINVAL)")
            out.copy_(x[:, sel::2])


def split_bwd(mode, g_out, mask, gx, sel=0):
    _host(g_out, mask, gx)
    with torch.no_grad():
        if mode == MASK:
            gx.copy_(mask * g_out)
        else:
            gx[:, sel::2] = g_out
            gx[:, 1 - sel::2] = 0


def merge(mode, x, mask, shift, sign, y, sel=0):
    _host(x, mask, shift, y)
    with torch.no_grad():
        if mode == MASK:
            om = 1 - mask
            x1 = mask * x
            x2 = om * x
            sh = (sign * shift) * om
            y.copy_(x1 + (x2 + sh))
        else:
            on = 1 - sel
            out = x.clone()
            out[:, on::2] = x[:, on::2] + sign * shift
            y.copy_(out)


def merge_bwd(mode, gy, mask, sign, gx, gshift, sel=0):
    _host(gy, mask, gx, gshift)
    with torch.no_grad():
        if mode == MASK:
            om = 1 - mask
            gx.copy_(mask * gy + om * gy)
            gshift.copy_(sign * (gy * om))
        else:
            gx.copy_(gy)
            gshift.copy_(sign * gy[:, 1 - sel::2])


def scale_fwd(x, log_scale, sign, y, logdet):
    _host(x, log_scale, y, logdet)
    with torch.no_grad():
        f = torch.exp(sign * log_scale)
        res = x * f
        y.copy_(res)
        logdet.copy_(log_scale.sum())


def scale_bwd(gy, y, log_scale, g_logdet, sign, gx, g_log_scale):
    _host(gy, y, log_scale, g_logdet, gx, g_log_scale)
    with torch.no_grad():
        f = torch.exp(sign * log_scale)
        s = (gy * y).sum(0)
        g_log_scale.copy_(sign * s + (g_logdet if g_logdet is not None else 0))
        gx.copy_(gy * f)


def made_fwd(x, net, u, logdet):
    _host(x, net, u, logdet)
    D = x.shape[1]
    with torch.no_grad():
        m, loga = net[:, :D], net[:, D:]
        u.copy_((x - m) * torch.exp(-loga))
        logdet.copy_(-loga)


def made_bwd(gu, gld, x, net, gx, gnet):
    _host(gu, gld, x, net, gx, gnet)
    D = x.shape[1]
    with torch.no_grad():
        m, loga = net[:, :D], net[:, D:]
        gu_ = torch.zeros_like(x) if gu is None else gu
        gld_ = torch.zeros_like(x) if gld is None else gld
        e = torch.exp(-loga)
        u = (x - m) * e
        g = gu_ * e
        gx.copy_(g)
        gnet[:, :D] = -g
        gnet[:, D:] = -(gu_ * u) - gld_


def made_inv_col(u, net, x, col):
    _host(u, net, x)
    D = u.shape[1]
    with torch.no_grad():
        x[:, col] = u[:, col] * torch.exp(net[:, D + col]) + net[:, col]


def _lp(base, z, loc, scale):
    if base == NORMAL:
        c = -0.5 * math.log(2 * math.pi)
        diff = z - loc
        prec = 1 / (scale * scale)
        return (c - torch.log(scale)) - 0.5 * prec * (diff * diff)
    at = ((z - loc) / scale).abs()
    return -(at + 2 * torch.log1p(torch.exp(-at))) - torch.log(scale)


def _dz(base, z, loc, scale):
    if base == NORMAL:
        return -((1 / (scale * scale)) * (z - loc))
    t = (z - loc) / scale
    return -(torch.tanh(0.5 * t) / scale)


def tail(base, z, loc, scale, param_rows, logdet, logdet_kind, out):
    _host(z, loc, scale, logdet, out)
    with torch.no_grad():
        s = _lp(base, z, loc, scale).sum(1)
        if logdet_kind == LOGDET_SCALAR:
            s = s + logdet.reshape(())
        elif logdet_kind == LOGDET_ROWS:
            s = s + logdet
        out.copy_(s)


def tail_bwd(base, g, z, loc, scale, param_rows, gz, g_logdet):
    _host(g, z, loc, scale, gz, g_logdet)
    with torch.no_grad():
        gz.copy_(g[:, None] * _dz(base, z, loc, scale))
        if g_logdet is not None:
            g_logdet.copy_(g)


router = host_routing.Router("zhusuan._flow_hip", {n: globals()[n] for n in NAMES})
install, uninstall, count_launches = router.install, router.uninstall, router.count
# the suite's ``dev`` fixture (host and hip) with the flow kernels routed accordingly: imported by the tests
fdev = host_routing.dev_fixture("fdev", router)
