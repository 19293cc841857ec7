"""TEST INFRASTRUCTURE, companion of tests/cat_host.py for MultivariateNormalCholesky: ``install()`` replaces the functions of
the binding (``zhusuan._mvn_hip.sample_logprob`` ... ``logprob_bwd``) by torch restatements of the kernel contract of
include/zs_mvn.h on CPU tensors, so that the host logic of the distribution (shapes, broadcasting, caching, autograd wiring, draw
order, call ids, launch budget) runs on a GPU-less machine.  The package itself contains no such routing.

The restatements evaluate the header's formulas in float64 and round the results to the tensors' dtype.  Where no noise is
injected, the normals are flat elements of the C oracle's ``zs_philox_normal_f32`` stream for the launch's (seed, call): the
kernels' noise contract.  ``recording()`` lists every launch (tests/host_routing.py).

``reference_*`` are the same formulas in pure float64 on float64 inputs: the truth of the kernel and distribution tests.  They
read the lower triangle only (``torch.tril``)."""
import math

import torch

import host_routing

F64 = torch.float64
LOG_2PI = math.log(2.0 * math.pi)


def philox_normal(n, seed, call, rng_state=None):
    return host_routing.philox("zs_philox_normal_f32", n, seed, call, rng_state)


# ------------------------------------------------------------------------------------------------ the float64 truth
def lower(tril):
    """L in float64 with an exactly zero upper triangle, whatever the input holds there (NaN included)."""
    L = tril.to(F64)
    mask = torch.ones(L.shape[-2:], dtype=torch.bool).tril()
    return torch.where(mask, L, torch.zeros_like(L))


def reference_density(tril, y):
    """lp[k,r] = -D/2 log 2 pi - sum_i log L_ii - 1/2 sum_i y_i^2.  y [K, R, D]."""
    L = lower(tril)
    D = L.shape[-1]
    return -0.5 * D * LOG_2PI - torch.log(torch.diagonal(L, dim1=-2, dim2=-1)).sum(-1)[None] - 0.5 * (y.to(F64) ** 2).sum(-1)


def reference_sample(mean, tril, eps):
    """(z [K, R, D], lp [K, R]) of z = mean + L eps."""
    L = lower(tril)
    z = mean.to(F64)[None] + torch.einsum("rij,krj->kri", L, eps.to(F64))
    return z, reference_density(tril, eps)


def reference_whiten(mean, tril, x):
    """y = L^-1 (x - mean).  x [K, R, D]."""
    L = lower(tril)
    diff = (x.to(F64) - mean.to(F64)[None])[..., None]
    return torch.linalg.solve_triangular(L[None].expand(diff.shape[0], -1, -1, -1), diff, upper=False)[..., 0]


def reference_back(tril, y):
    """w = L^-T y.  y [K, R, D]."""
    L = lower(tril)
    return torch.linalg.solve_triangular(L.transpose(-1, -2)[None].expand(y.shape[0], -1, -1, -1), y.to(F64)[..., None],
                                         upper=True)[..., 0]


def reference_logprob(mean, tril, x):
    return reference_density(tril, reference_whiten(mean, tril, x))


def reference_score(tril, y, glp):
    """(w, gmean, gtril) of the density's direct dependence at y: w = L^-T y, gmean = sum_k g w, gtril = sum_k g (w y^T - diag(1 / L_ii)),
    lower triangle."""
    L = lower(tril)
    w = reference_back(tril, y)
    g = glp.to(F64)
    gmean = (g[..., None] * w).sum(0)
    outer = torch.einsum("kr,kri,krj->rij", g, w, y.to(F64))
    gtril = outer - torch.diag_embed(g.sum(0)[:, None] / torch.diagonal(L, dim1=-2, dim2=-1))
    return w, gmean, torch.tril(gtril)


def reference_sample_bwd(tril, eps, gz, glp):
    """(gmean, gtril) of the reparameterised draw."""
    L = lower(tril)
    gmean = gz.to(F64).sum(0)
    gtril = torch.einsum("kri,krj->rij", gz.to(F64), eps.to(F64))
    gtril = gtril - torch.diag_embed(glp.to(F64).sum(0)[:, None] / torch.diagonal(L, dim1=-2, dim2=-1))
    return gmean, torch.tril(gtril)


# ------------------------------------------------------------------------------------------------ the routed binding
def _normals(tril, K, eps, seed, call, rng_state):
    R, D, _ = tril.shape
    if eps is not None:
        return eps.reshape(K, R, D)
    return philox_normal(K * R * D, seed, call, rng_state).reshape(K, R, D)


def _rows(x, K, R, D):
    return x.reshape(-1, R, D).expand(K, R, D)


def sample_logprob(mean, tril, K, eps=None, seed=0, call=0, rng_state=None):
    host_routing.host_only("mvn_host", [mean, tril, eps, rng_state])
    with torch.no_grad():
        z, lp = reference_sample(mean, tril, _normals(tril, K, eps, seed, call, rng_state))
    return z.to(mean.dtype), lp.to(mean.dtype)


def sample_logprob_bwd(tril, K, reparameterized, eps=None, seed=0, call=0, rng_state=None, gz=None, glp=None, want_gmean=True,
                       want_gtril=True):
    host_routing.host_only("mvn_host", [tril, eps, gz, glp, rng_state])
    R, D, _ = tril.shape
    with torch.no_grad():
        e = _normals(tril, K, eps, seed, call, rng_state)
        g = torch.zeros(K, R, dtype=F64) if glp is None else glp.reshape(K, R)
        if reparameterized:
            gzz = torch.zeros(K, R, D, dtype=F64) if gz is None else gz.reshape(K, R, D)
            gmean, gtril = reference_sample_bwd(tril, e, gzz, g)
        else:
            _, gmean, gtril = reference_score(tril, e, g)
    return (gmean.to(tril.dtype) if want_gmean else None), (gtril.to(tril.dtype) if want_gtril else None)


def logprob(mean, tril, K, x):
    host_routing.host_only("mvn_host", [mean, tril, x])
    R, D, _ = tril.shape
    with torch.no_grad():
        return reference_logprob(mean, tril, _rows(x, K, R, D)).to(mean.dtype)


def logprob_bwd(mean, tril, K, x, glp, want_gx=True, want_gmean=True, want_gtril=True):
    host_routing.host_only("mvn_host", [mean, tril, x, glp])
    R, D, _ = tril.shape
    with torch.no_grad():
        y = reference_whiten(mean, tril, _rows(x, K, R, D))
        g = glp.reshape(K, R)
        w, gmean, gtril = reference_score(tril, y, g)
        gx = (-g.to(F64)[..., None] * w).to(mean.dtype) if want_gx else None
    return gx, (gmean.to(mean.dtype) if want_gmean else None), (gtril.to(mean.dtype) if want_gtril else None)


router = host_routing.Router("zhusuan._mvn_hip", {
    "sample_logprob": sample_logprob, "sample_logprob_bwd": sample_logprob_bwd, "logprob": logprob, "logprob_bwd": logprob_bwd})
install, uninstall, recording = router.install, router.uninstall, router.recording
# the suite's ``dev`` fixture (host and hip) with the multivariate-normal binding routed accordingly: imported by the tests
vdev = host_routing.dev_fixture("vdev", router)
