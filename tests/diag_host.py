"""TEST INFRASTRUCTURE, companion of tests/klpq_host.py for the chain diagnostics: ``install()`` replaces the two functions of the
binding (``zhusuan._diag_hip.summary`` / ``autocorr``) by torch restatements of the kernel contract of include/zs_diag.h on CPU
tensors, so that the host logic of ``zhusuan.diagnostics`` (shapes, strides, chain axes, the trace) runs on a GPU-less machine.  The
package itself contains no such routing.

The restatements evaluate the header's formulas in float64 and round the results to the tensors' dtype.  ``recording()`` lists every
launch (tests/host_routing.py).  ``reference_*`` are the same formulas in pure float64 on float64 inputs: the truth of the kernel
and interface tests.  ``recipe`` is the one input recipe of every level of test."""
import math

import numpy as np
import torch

import host_routing

F64 = torch.float64
OUTPUTS = ("mean", "var_plus", "rhat", "ess", "lags", "capped")
MIN_P = 1e-9          # the float64 truth of every case must keep every pair sum it examined at least this far from zero


# ------------------------------------------------------------------------------------------------ the input recipe
def recipe(T, C, E, case=0):
    """float32 AR(1) draws [T, C, E] (numpy): x_t = phi_e x_{t-1} + z_t with phi = linspace(-0.5, 0.9, E), the last chain shifted
    by +0.25; seed default_rng(1000 T + 10 C + case)."""
    rng = np.random.default_rng(1000 * T + 10 * C + case)
    phi = np.linspace(-0.5, 0.9, E).astype(np.float32)
    z = rng.standard_normal((T, C, E)).astype(np.float32)
    x = np.empty((T, C, E), dtype=np.float32)
    x[0] = z[0]
    for t in range(1, T):
        x[t] = phi * x[t - 1] + z[t]
    x[:, C - 1] += np.float32(0.25)
    return x


# ------------------------------------------------------------------------------------------------ the float64 truth
def chains_of(x, split):
    """[T, C, E] -> [M, N, E]: with ``split`` all first halves in chain order, then all second halves."""
    T = x.shape[0]
    if split:
        N = T // 2
        x = torch.cat([x[:N], x[T - N:]], 1)
    return x.permute(1, 0, 2)


def reference_summary(x, split, max_lag):
    """The header's steps 1 - 8 on a float64 [T, C, E] tensor.  dict of [E] tensors: the six outputs (lags, capped int32), and
    for the tests' bounds ``tau``, ``W``, ``absx`` (the mean of |x| over the draws that entered), ``kappa`` (the largest
    sum_t (x - mean_m)^2 / (N W) over m), ``gamma0`` (mean_m sum_t d_t^2 / N) and ``min_abs_p`` (the smallest |P_k| examined,
    +inf where no pair was)."""
    x = x.to(F64)
    X = chains_of(x, split)
    M, N, E = X.shape
    mean_m = X.sum(1) / N
    d = X - mean_m[:, None]
    ss = (d * d).sum(1)
    W = (ss / (N - 1)).sum(0) / M
    mean = mean_m.sum(0) / M
    BN = ((mean_m - mean) ** 2).sum(0) / (M - 1) if M > 1 else torch.zeros(E, dtype=F64)
    varp = (N - 1) / N * W + BN
    finite = torch.isfinite(X).all(0).all(0)
    live = finite & (W != 0)
    nan = torch.full((E,), math.nan, dtype=F64)
    Lcap = N - 1 if (max_lag is None or max_lag < 0) else min(int(max_lag), N - 1)
    tau = torch.full((E,), -1.0, dtype=F64)
    prev = torch.full((E,), math.inf, dtype=F64)
    lags = torch.zeros(E, dtype=torch.int32)
    capped = live.to(torch.int32)
    min_abs_p = torch.full((E,), math.inf, dtype=F64)
    active = live.clone()
    k = 0
    while 2 * k + 1 <= Lcap and bool(active.any()):
        idx = active.nonzero().reshape(-1)
        dd = d[:, :, idx]
        P = 0.0
        for l in (2 * k, 2 * k + 1):
            g = (dd[:, :N - l] * dd[:, l:]).sum(1) / N
            P = P + (1.0 - (W[idx] - g.sum(0) / M) / varp[idx])
        min_abs_p[idx] = torch.minimum(min_abs_p[idx], P.abs())
        go = P > 0
        stop = idx[~go]
        capped[stop] = 0
        active[stop] = False
        keep = idx[go]
        Pm = torch.minimum(P[go], prev[keep])
        prev[keep] = Pm
        tau[keep] += 2.0 * Pm
        lags[keep] = 2 * (k + 1)
        k += 1
    floor = 1.0 / math.log10(M * N)
    tau = torch.clamp(tau, min=floor)
    with np.errstate(all="ignore"):
        rhat = torch.where(live, torch.sqrt(varp / torch.where(live, W, torch.ones_like(W))), nan)
    entering = X.abs().sum(0).sum(0) / (M * N)
    return dict(mean=torch.where(finite, mean, nan), var_plus=torch.where(finite, varp, nan), rhat=rhat,
                ess=torch.where(live, M * N / tau, nan), lags=lags, capped=capped, tau=tau, W=W, absx=entering,
                kappa=torch.where(live, ss.max(0).values / (N * torch.where(live, W, torch.ones_like(W))), nan),
                gamma0=ss.sum(0) / (M * N), min_abs_p=min_abs_p, N=N, M=M)


def reference_autocorr(x, L):
    """acf [L + 1, C, E] of the unsplit chains of a float64 [T, C, E] tensor."""
    x = x.to(F64)
    T = x.shape[0]
    d = x - x.sum(0) / T
    g = torch.stack([(d[:T - l] * d[l:]).sum(0) / T for l in range(L + 1)])
    return g / g[0]


# ------------------------------------------------------------------------------------------------ the routed binding
def _view(x, st, sc, T, C, E):
    """the operand as the kernel addresses it: x[t st + c sc + e] (with one chain sc is never stepped)"""
    return torch.as_strided(x, (T, C, E), (st, sc if C > 1 else 0, 1), x.storage_offset())


def summary(x, st, sc, T, C, E, split, max_lag, want=OUTPUTS):
    host_routing.host_only("diag_host", [x])
    with torch.no_grad():
        r = reference_summary(_view(x, st, sc, T, C, E), split, max_lag)
    return tuple(None if n not in want else (r[n] if n in ("lags", "capped") else r[n].to(x.dtype)) for n in OUTPUTS)


def autocorr(x, st, sc, T, C, E, L):
    host_routing.host_only("diag_host", [x])
    with torch.no_grad():
        return reference_autocorr(_view(x, st, sc, T, C, E), L).to(x.dtype)


router = host_routing.Router("zhusuan._diag_hip", {"summary": summary, "autocorr": autocorr})
install, uninstall, recording = router.install, router.uninstall, router.recording
# the suite's ``dev`` fixture (host and hip) with the diagnostics binding routed accordingly: imported by the tests
ddev = host_routing.dev_fixture("ddev", router)
