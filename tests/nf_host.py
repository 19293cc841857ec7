"""TEST INFRASTRUCTURE, companion of tests/mvn_host.py for ``zhusuan.transform``: ``install()`` replaces the functions of the
binding (``zhusuan._nf_hip.planar_fwd`` ... ``householder_bwd``) by torch restatements of the kernel contract of include/zs_nf.h
on CPU tensors, so that the host logic of the modules (shapes, chunking, autograd wiring, NULL operands, launch budget) runs on a
GPU-less machine.  The package itself contains no such routing.

The restatements evaluate the header's formulas in float64 and round the results to the tensors' dtype; the host ``planar_bwd``
returns the row sums as the partials of ONE workgroup.  ``recording()`` (tests/host_routing.py) wraps the five functions the binding
holds at that moment -- the restatements on the host, the real ones on the GPU -- and lists every call as ``(name, args, kwargs)``
with each tensor replaced by its shape: the launch budget and the NULL operands of the modules read the same way on both.

``reference_*`` are the same formulas in pure float64 on float64 inputs: the truth of the kernel and module tests."""
import torch
import torch.nn.functional as F

import host_routing

F64 = torch.float64


# ------------------------------------------------------------------------------------------------ the float64 truth
def reference_planar_params(u, w):
    """(s, n, k, uh, c) per layer: s, n, k, c [L], uh [L, D]."""
    u, w = u.to(F64), w.to(F64)
    s, n = (w * u).sum(1), (w * w).sum(1)
    k = F.softplus(s) - 1.0 - s
    uh = u + (k / n)[:, None] * w
    return s, n, k, uh, (w * uh).sum(1)


def reference_planar_fwd(u, w, b, x, keep=False):
    """(y [R, D], logdet [R]); with ``keep`` also the layer inputs z_l and the tanh values t_l."""
    _, _, _, uh, c = reference_planar_params(u, w)
    w, b, z = w.to(F64), b.to(F64), x.to(F64)
    ld = torch.zeros(z.shape[0], dtype=F64)
    zs, ts = [], []
    for l in range(u.shape[0]):
        t = torch.tanh(z @ w[l] + b[l])
        zs.append(z), ts.append(t)
        z = z + uh[l] * t[:, None]
        ld = ld + torch.log(torch.abs(1.0 + (1.0 - t * t) * c[l]))
    return (z, ld, zs, ts) if keep else (z, ld)


def reference_planar_bwd(u, w, b, x, gy=None, gld=None):
    """(gx [R, D], Guh [L, D], Gw [L, D], Gb [L], Gc [L]): the row cotangent and the four row sums of P1b."""
    _, _, _, uh, c = reference_planar_params(u, w)
    _, _, zs, ts = reference_planar_fwd(u, w, b, x, keep=True)
    w = w.to(F64)
    (L, D), R = u.shape, x.shape[0]
    g = torch.zeros(R, D, dtype=F64) if gy is None else gy.to(F64).clone()
    gl = torch.zeros(R, dtype=F64) if gld is None else gld.to(F64)
    Guh, Gw, Gb, Gc = torch.zeros(L, D, dtype=F64), torch.zeros(L, D, dtype=F64), torch.zeros(L, dtype=F64), torch.zeros(L, dtype=F64)
    for l in range(L - 1, -1, -1):
        t = ts[l]
        h = 1.0 - t * t
        m = 1.0 + h * c[l]
        ga = (g @ uh[l] + gl * (c[l] / m) * (-2.0 * t)) * h
        Guh[l], Gw[l], Gb[l], Gc[l] = (g * t[:, None]).sum(0), (ga[:, None] * zs[l]).sum(0), ga.sum(), (gl * h / m).sum()
        g = g + ga[:, None] * w[l]
    return g, Guh, Gw, Gb, Gc


def reference_planar_finish(u, w, Guh, Gw, Gb, Gc):
    """(gu, gw, gb): the parameter chain of P1f."""
    s, n, k, uh, _ = reference_planar_params(u, w)
    u, w = u.to(F64), w.to(F64)
    Guh = Guh.to(F64) + Gc.to(F64)[:, None] * w
    Gw = Gw.to(F64) + Gc.to(F64)[:, None] * uh
    p = (Guh * w).sum(1)
    dk = torch.sigmoid(s) - 1.0
    gu = Guh + ((p / n) * dk)[:, None] * w
    gw = Gw + Guh * (k / n)[:, None] + ((p / n) * dk)[:, None] * u - (2.0 * k * p / (n * n))[:, None] * w
    return gu, gw, Gb.to(F64)


def reference_householder_fwd(v, x, keep=False):
    v, z = v.to(F64), x.to(F64)
    zs = []
    for l in range(v.shape[0]):
        zs.append(z)
        z = z - 2.0 * v[l] * ((v[l] * z).sum(1, keepdim=True) / (v[l] * v[l]).sum(1, keepdim=True))
    return (z, zs) if keep else z


def reference_householder_bwd(v, x, gy):
    """(gx [R, D], gv [L, R, D])."""
    _, zs = reference_householder_fwd(v, x, keep=True)
    v, g = v.to(F64), gy.to(F64)
    gv = torch.zeros_like(v)
    for l in range(v.shape[0] - 1, -1, -1):
        n, p, q = ((v[l] * a).sum(1, keepdim=True) for a in (v[l], zs[l], g))
        gv[l] = -2.0 * (p * g + q * zs[l]) / n + 4.0 * p * q * v[l] / (n * n)
        g = g - 2.0 * v[l] * q / n
    return g, gv


# ------------------------------------------------------------------------------------------------ the routed binding
def planar_fwd(u, w, b, x, want_y=True, want_logdet=True):
    host_routing.host_only("nf_host", [u, w, b, x])
    with torch.no_grad():
        y, ld = reference_planar_fwd(u, w, b, x)
    return (y.to(x.dtype) if want_y else None), (ld.to(x.dtype) if want_logdet else None)


def planar_bwd(u, w, b, x, gy=None, gld=None, want_gx=True, want_partials=True):
    host_routing.host_only("nf_host", [u, w, b, x, gy, gld])
    assert gy is not None or gld is not None and (want_gx or want_partials)
    with torch.no_grad():
        gx, Guh, Gw, Gb, Gc = reference_planar_bwd(u, w, b, x, gy, gld)
        partials = torch.cat([Guh, Gw, Gb[:, None], Gc[:, None]], 1)[None].to(x.dtype)
    return (gx.to(x.dtype) if want_gx else None), (partials if want_partials else None)


def planar_finish(u, w, partials, want_gu=True, want_gw=True, want_gb=True):
    host_routing.host_only("nf_host", [u, w, partials])
    D = u.shape[1]
    with torch.no_grad():
        P = partials.to(F64).sum(0)
        gu, gw, gb = reference_planar_finish(u, w, P[:, :D], P[:, D:2 * D], P[:, 2 * D], P[:, 2 * D + 1])
    return (gu.to(u.dtype) if want_gu else None), (gw.to(u.dtype) if want_gw else None), (gb.to(u.dtype) if want_gb else None)


def householder_fwd(v, x):
    host_routing.host_only("nf_host", [v, x])
    with torch.no_grad():
        return reference_householder_fwd(v, x).to(x.dtype)


def householder_bwd(v, x, gy, want_gx=True, want_gv=True):
    host_routing.host_only("nf_host", [v, x, gy])
    with torch.no_grad():
        gx, gv = reference_householder_bwd(v, x, gy)
    return (gx.to(x.dtype) if want_gx else None), (gv.to(x.dtype) if want_gv else None)


router = host_routing.Router("zhusuan._nf_hip", {
    "planar_fwd": planar_fwd, "planar_bwd": planar_bwd, "planar_finish": planar_finish, "householder_fwd": householder_fwd,
    "householder_bwd": householder_bwd})
install, uninstall, recording = router.install, router.uninstall, router.recording
# the suite's ``dev`` fixture (host and hip) with the flow-stack binding routed accordingly: imported by the tests
ndev = host_routing.dev_fixture("ndev", router)
