"""TEST INFRASTRUCTURE, companion of tests/host_backend.py for ``zhusuan.mcmc``: ``install()`` replaces the single update
function of the sampler binding (``zhusuan._mcmc_hip.update``) by a torch restatement of the kernel contract of
include/zs_mcmc.h on CPU tensors, so that the samplers' host logic (latent discovery, draw order, launch grouping, state
buffers, call ids) runs on a GPU-less machine.  The package itself contains no such routing.

The restatement is written in the tensors' own dtype in the operation order of the header.  Where a tensor brings no injected
noise its standard normals are flat elements [start, start + numel) of the C oracle's ``zs_philox_normal_f32`` stream for the
launch's (seed, call): the kernel's noise contract."""
import math

import torch

import host_routing

SGLD, PSGLD, SGHMC_PRE, SGHMC_POST = 0, 1, 2, 3
SECOND_ORDER, RESAMPLE_V = 1, 2
MAX_TENSORS = 32


def philox_normal(n, seed, call, rng_state=None):
    """Elements [0, n) of the oracle's Philox normal stream (float32, CPU)."""
    return host_routing.philox("zs_philox_normal_f32", n, seed, call, rng_state)


def update(kind, q_in, q_out, grad=None, state=None, z=None, lr=0., decay=0., epsilon=0., alpha=0., beta=0., flags=0,
           seed=0, call=0, rng_state=None, library=None):
    if len(q_in) > MAX_TENSORS:
        raise RuntimeError("zs_mcmc_update failed with code -2: not supported (ZS_ENOTSUP)")
    if not q_in:
        return
    host_routing.host_only("mcmc_host", [q_in, q_out, grad or [], state or [], z or []])
    second, resample = bool(flags & SECOND_ORDER), bool(flags & RESAMPLE_V)
    draws = kind != SGHMC_PRE or resample
    sizes = [q.numel() for q in q_in]
    n = sum(sizes)
    stream = None
    if draws and (z is None or any(u is None for u in z)):
        stream = philox_normal(n, seed, call, rng_state)
    start = 0
    with torch.no_grad():
        for i, q in enumerate(q_in):
            dt = q.dtype
            if draws:
                zi = z[i] if z is not None and z[i] is not None else stream[start:start + sizes[i]].view(q.shape).to(dt)
                zi = zi.reshape(q.shape)
            g = grad[i].reshape(q.shape) if grad is not None else None
            s = state[i] if state is not None else None
            if kind == SGLD:
                new = q + (0.5 * lr) * g + math.sqrt(lr) * zi
            elif kind == PSGLD:
                a = decay * s + (1.0 - decay) * (g * g)
                G = 1.0 / (epsilon + torch.sqrt(a))
                new = q + ((0.5 * lr) * G) * g + torch.sqrt(lr * G) * zi
                s.copy_(a)
            elif kind == SGHMC_PRE:
                if resample:
                    s.copy_((math.sqrt(lr) * zi).reshape(s.shape))
                new = q + 0.5 * s.reshape(q.shape) if second else q.clone()
            elif kind == SGHMC_POST:
                noise = math.sqrt(2.0 * (alpha - beta) * lr)
                v = s.reshape(q.shape)
                if second:
                    d = math.exp(-0.5 * alpha)
                    v = d * (d * v + lr * g + noise * zi)
                    new = q + 0.5 * v
                else:
                    v = (1.0 - alpha) * v + lr * g + noise * zi
                    new = q + v
                s.copy_(v.reshape(s.shape))
            else:
                raise RuntimeError("zs_mcmc_update failed with code -1: invalid argument (ZS_EINVAL)")
            q_out[i].copy_(new.reshape(q_out[i].shape))
            start += sizes[i]


router = host_routing.Router("zhusuan._mcmc_hip", {"update": update})
install, uninstall = router.install, router.uninstall
# the suite's ``dev`` fixture (host and hip) with the samplers' update routed accordingly: imported by the tests
mdev = host_routing.dev_fixture("mdev", router)
