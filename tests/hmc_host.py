"""TEST INFRASTRUCTURE, companion of tests/mcmc_host.py for ``zhusuan.mcmc.HMC``: ``install()`` replaces the three functions of
the binding (``zhusuan._hmc_hip.move`` / ``decide`` / ``select``) by torch restatements of the kernel contract of
include/zs_hmc.h on CPU tensors, so that the sampler's host logic (chain shape, draw order, chunking, call ids, launch budget,
in-place results) runs on a GPU-less machine.  The package itself contains no such routing.

The restatement is written in the tensors' own dtype in the operation order of the header (torch has no fused multiply-add:
the leapfrog's a + b * c rounds twice where the kernel rounds once); the kinetic sum of a (tensor, chain) goes, in that dtype,
into the first of the tensor's slots of the workspace and zeros into the others; ``decide`` is in float64.  Where a tensor
brings no injected noise its momenta are flat elements of the C oracle's ``zs_philox_normal_f32`` stream for the launch's
(seed, call), and ``u`` those of ``zs_philox_uniform_f32``: the kernels' noise contract.

``reference_iteration`` is a pure float64 HMC iteration (no workspace, no state block): the truth of the sampler tests."""
import math

import torch

import host_routing


BEGIN, STEP, END = 0, 1, 2
MAX_TENSORS, MAX_CHUNKS, TILE = 32, 16, 1024
EPS, EPS_INIT, M, HBAR, LOG_EPS, LOG_EPSBAR, ABAR, NACC = range(8)


def philox_normal(n, seed, call, rng_state=None):
    """Elements [0, n) of the oracle's Philox normal stream (float32, CPU)."""
    return host_routing.philox("zs_philox_normal_f32", n, seed, call, rng_state)


def philox_uniform(n, seed, call, rng_state=None):
    return host_routing.philox("zs_philox_uniform_f32", n, seed, call, rng_state)


def pieces(row):
    return (int(row) + TILE - 2) // TILE + 1


def move(kind, n_chains, state, q, p, grad, q0=None, z=None, p0=None, ksum=None, seed=0, call=0, rng_state=None, library=None):
    if len(q) > MAX_TENSORS:
        raise RuntimeError("zs_hmc_move failed with code -2: not supported (ZS_ENOTSUP)")
    if not q:
        return
    if kind not in (BEGIN, STEP, END):
        raise RuntimeError("zs_hmc_move failed with code -1: invalid argument (ZS_EINVAL)")
    host_routing.host_only("hmc_host", list(q) + list(p) + list(grad) + list(q0 or []) + list(z or []) + list(p0 or []) + [state, ksum, rng_state])
    C = int(n_chains)
    sizes = [t.numel() for t in q]
    rows = [k // C for k in sizes]
    slots = sum(pieces(r) for r in rows)
    dt = q[0].dtype
    eps = float(state[EPS])
    e, h = torch.tensor(eps, dtype=torch.float64).to(dt), torch.tensor(0.5 * eps, dtype=torch.float64).to(dt)
    stream = None
    if kind == BEGIN and (z is None or any(t is None for t in z)):
        stream = philox_normal(sum(sizes), seed, call, rng_state)
    ks = ksum.view(C, slots) if kind != STEP else None
    if ks is not None:
        ks.zero_()
    start = poff = 0
    with torch.no_grad():
        for i in range(len(q)):
            g = grad[i].reshape(q[i].shape)
            if kind == BEGIN:
                zi = z[i] if z is not None and z[i] is not None else stream[start:start + sizes[i]].to(dt)
                zi = zi.reshape(q[i].shape)
                pn = zi + h * g
                q[i].copy_(q0[i] + e * pn)
                p[i].copy_(pn)
                if p0 is not None and p0[i] is not None:
                    p0[i].copy_(zi)
                sq = zi * zi
            elif kind == STEP:
                p[i].copy_(p[i] + e * g)
                q[i].copy_(q[i] + e * p[i])
            else:
                pl = p[i] + h * g
                sq = pl * pl
            if kind != STEP:
                ks[:, poff] = sq.reshape(C, rows[i]).sum(dim=1)
            start += sizes[i]
            poff += pieces(rows[i])


def decide_math(k0, k1, logp0, logp1, u, state, adapting, delta, gamma, t0, kappa):
    """float64 restatement of decide on (k0, k1, logp0, logp1, u: float64[C]) and a state list; returns
    (accept bool[C], a, dH, new state list)."""
    dh = (logp1 - logp0) - (k1 - k0)
    fin = torch.isfinite(dh)
    a = torch.where(fin, torch.exp(torch.clamp(dh, max=0.0)), torch.zeros_like(dh))
    acc = fin & (torch.log(u) < dh)
    abar = float(a.sum()) / a.numel()
    st = list(state)
    if adapting:
        m = st[M] + 1.0
        w = 1.0 / (m + t0)
        hbar = (1.0 - w) * st[HBAR] + w * (delta - abar)
        log_eps = math.log(10.0 * st[EPS_INIT]) - (math.sqrt(m) / gamma) * hbar
        eta = m ** (-kappa)
        st[M], st[HBAR], st[LOG_EPS] = m, hbar, log_eps
        st[LOG_EPSBAR] = eta * log_eps + (1.0 - eta) * st[LOG_EPSBAR]
        st[EPS] = math.exp(log_eps)
    elif st[M] > 0.0:
        st[EPS] = math.exp(st[LOG_EPSBAR])
    st[ABAR] = abar
    st[NACC] = float(acc.sum())
    return acc, a, dh, st


def decide(chunks, n_chains, logp0, logp1, u, state, out, accept, adapting, delta, gamma, t0, kappa, seed=0, call=0,
           rng_state=None, library=None):
    if len(chunks) > MAX_CHUNKS:
        raise RuntimeError("zs_hmc_decide failed with code -2: not supported (ZS_ENOTSUP)")
    C = int(n_chains)
    host_routing.host_only("hmc_host", [logp0, logp1, u, state, out, accept, rng_state] + [t for c in chunks for t in c[:2]])
    k0 = sum(c[0].view(C, c[2]).double().sum(dim=1) for c in chunks) * 0.5
    k1 = sum(c[1].view(C, c[2]).double().sum(dim=1) for c in chunks) * 0.5
    uu = u.double() if u is not None else philox_uniform(C, seed, call, rng_state).double()
    l0, l1 = logp0.double(), logp1.double()
    acc, a, dh, st = decide_math(k0, k1, l0, l1, uu, state.tolist(), adapting, delta, gamma, t0, kappa)
    accept.copy_(acc.to(torch.int32))
    o = out.view(5, C)
    o[0], o[1], o[2], o[3], o[4] = a, k0 - l0, k1 - l1, dh, torch.where(acc, l1, l0)
    state.copy_(torch.tensor(st, dtype=torch.float64))


def select(n_chains, q0, q, q_out, accept, library=None):
    if not q:
        return
    host_routing.host_only("hmc_host", list(q0) + list(q) + list(q_out) + [accept])
    C = int(n_chains)
    with torch.no_grad():
        for a, b, o in zip(q0, q, q_out):
            m = accept.bool().view([C] + [1]).expand(C, a.numel() // C)
            o.copy_(torch.where(m, b.reshape(C, -1), a.reshape(C, -1)).reshape(o.shape))


router = host_routing.Router("zhusuan._hmc_hip", {"move": move, "decide": decide, "select": select})
install, uninstall = router.install, router.uninstall


# ------------------------------------------------------------------------------------------------ the float64 truth
def reference_iteration(logp_and_grad, q0, z, u, eps, n_leapfrogs):
    """One HMC iteration in the arithmetic of the tensors given (float64 for the truth; float32 tensors give the reference's
    own float32 distance).  ``logp_and_grad(list of tensors) -> (logp [C], list of gradients)``; ``q0`` / ``z``: lists of
    tensors whose first dimension is the chain; ``u``: [C].  Returns a dict: q (selected), accept, a, dh, h0, h1, logp0, logp1."""
    C = u.numel()
    dt = q0[0].dtype
    e = torch.tensor(eps, dtype=torch.float64).to(dt)
    h = torch.tensor(0.5 * eps, dtype=torch.float64).to(dt)
    logp0, g = logp_and_grad(q0)
    k0 = 0.5 * sum((t * t).reshape(C, -1).sum(dim=1) for t in z).double()
    p = [t + h * gi for t, gi in zip(z, g)]
    q = [a + e * b for a, b in zip(q0, p)]
    for _ in range(n_leapfrogs - 1):
        _, g = logp_and_grad(q)
        p = [a + e * gi for a, gi in zip(p, g)]
        q = [a + e * b for a, b in zip(q, p)]
    logp1, g = logp_and_grad(q)
    pl = [a + h * gi for a, gi in zip(p, g)]
    k1 = 0.5 * sum((t * t).reshape(C, -1).sum(dim=1) for t in pl).double()
    l0, l1 = logp0.double().view(-1), logp1.double().view(-1)
    acc, a, dh, _ = decide_math(k0, k1, l0, l1, u.double().view(-1), [eps, eps, 0, 0, 0, 0, 0, 0], False, 0.8, 0.05, 100., 0.75)
    sel = [torch.where(acc.view([C] + [1] * (a_.dim() - 1)), b_, a_) for a_, b_ in zip(q0, q)]
    return dict(q=sel, accept=acc, a=a, dh=dh, h0=k0 - l0, h1=k1 - l1, logp0=l0, logp1=l1)


# the suite's ``dev`` fixture (host and hip) with the HMC binding routed accordingly: imported by the tests
hdev = host_routing.dev_fixture("hdev", router)
