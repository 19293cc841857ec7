"""Hamiltonian Monte Carlo with a Metropolis correction and dual-averaging step-size adaptation.

The reference (thuwzy/ZhuSuan-PyTorch) ships no HMC; its test/mcmc/test_mcmc.py carries the intended call, commented out:
``mcmc.HMC(step_size=0.01, n_leapfrogs=10)`` and ``sampler.sample(model, {}, {'x': x})[0]['x']``.  This is that sampler.  One
iteration is L + 1 evaluations of the log joint and its gradient through the existing kernels and, per chunk of latents,
L + 3 launches of lib/libzs_hmc.so (csrc/zs_hmc.hip, include/zs_hmc.h): BEGIN, L - 1 STEP, END, decide, select.  The step
size lives in a device-resident state block that the kernels read and ``decide`` updates: ``sample`` never synchronises the
host."""
import collections

import torch

from .. import _hmc_hip, _rng
from ._chunks import Chunk, plan_chunks

__all__ = [
    "HMC", "HMCInfo"
]

HMCInfo = collections.namedtuple("HMCInfo", ["samples", "acceptance_rate", "updated_step_size", "init_momentum",
                                             "orig_hamiltonian", "hamiltonian", "orig_log_prob", "log_prob"])

# chunk j of an iteration draws its momenta from call id + j * _CHUNK_CALL_STRIDE of the iteration's first id: one id per
# iteration whatever the number of chunks, and no two chunks on one stream
_CHUNK_CALL_STRIDE = 1 << 40


class _Chunk(Chunk):
    """The latents of one launch: at most _hmc_hip.MAX_TENSORS tensors of one dtype, forming one flat index space."""

    def __init__(self, idx, shapes, dtype, n_chains):
        super().__init__(idx, shapes, dtype)
        self.slots = _hmc_hip.ksum_slots([k // n_chains for k in self.sizes])


class HMC(object):
    """
    Hamiltonian Monte Carlo (unit mass) with per-chain accept / reject::

        hmc = zs.mcmc.HMC(step_size=0.1, n_leapfrogs=10, adapt_step_size=True)
        latent = {'w': w0}
        for it in range(n_iters):
            latent, info = hmc.sample(net, {'x': x, 'y': y}, latent)

    :param step_size: initial leapfrog step size.
    :param n_leapfrogs: leapfrog steps per iteration.
    :param adapt_step_size: run dual averaging (Hoffman & Gelman 2014) on the step size; a settable attribute: once set to
        False the averaged step size is used, frozen.
    :param target_acceptance_rate, gamma, t0, kappa: parameters of the dual averaging.
    :param adapt_mass: not implemented (unit mass only).
    """

    def __init__(self, step_size=1., n_leapfrogs=10, adapt_step_size=False, target_acceptance_rate=0.8, gamma=0.05, t0=100,
                 kappa=0.75, adapt_mass=False):
        if adapt_mass:
            raise NotImplementedError("zhusuan.mcmc.HMC: mass adaptation is not implemented (adapt_mass=True); unit mass only")
        if not step_size > 0:
            raise ValueError("step_size must be positive")
        if int(n_leapfrogs) < 1:
            raise ValueError("n_leapfrogs must be at least 1")
        self.n_leapfrogs = int(n_leapfrogs)
        self.adapt_step_size = bool(adapt_step_size)
        self.target_acceptance_rate = float(target_acceptance_rate)
        self.gamma = float(gamma)
        self.t0 = float(t0)
        self.kappa = float(kappa)
        self.t = 0
        self._initial_step_size = float(step_size)
        self._state = None           # float64[8] on the latents' device (include/zs_hmc.h)
        self._plan_key = None
        self._chunks = []

    @property
    def step_size(self):
        """The step size of the next iteration, read from the device (the only accessor that synchronises)."""
        if self._state is None:
            return self._initial_step_size
        return float(self._state[_hmc_hip.EPS])

    def initialize(self):
        self.t = 0

    # ------------------------------------------------------------------------------------------------ pieces of an iteration
    def _state_on(self, device):
        if self._state is None or self._state.device != device:
            self._state = torch.zeros(_hmc_hip.STATE_DOUBLES, dtype=torch.float64, device=device)
            self._state[:2].fill_(self._initial_step_size)
        return self._state

    def _plan(self, names, qs, n_chains):
        key = (tuple(names), tuple(tuple(q.shape) for q in qs), tuple(q.dtype for q in qs), n_chains)
        if key == self._plan_key:
            return self._chunks
        chunks = [_Chunk(part, [qs[i].shape for i in part], dtype, n_chains)
                  for dtype, part in plan_chunks(qs, lambda q: q.dtype, _hmc_hip.MAX_TENSORS)]
        if len(chunks) > _hmc_hip.MAX_CHUNKS:
            raise RuntimeError("zhusuan.mcmc.HMC: more than %d latents" % (_hmc_hip.MAX_CHUNKS * _hmc_hip.MAX_TENSORS))
        self._plan_key, self._chunks = key, chunks
        return chunks

    @staticmethod
    def _log_joint_and_grad(bn, observed, names, qs):
        """The log joint per chain at `qs` and the gradient of its sum: one forward with the latents observed, one
        ``autograd.grad`` through the existing kernels."""
        leaves = [q.detach().requires_grad_(True) for q in qs]
        bn.forward({**dict(zip(names, leaves)), **observed})
        log_joint = bn.log_joint()
        grads = torch.autograd.grad(log_joint.sum(), leaves)
        return log_joint.detach(), [g.contiguous() for g in grads]

    # ------------------------------------------------------------------------------------------------ one iteration
    def sample(self, bn, observed, latent, inplace=False):
        """
        One HMC iteration.

        :param bn: A instance of :class:`~zhusuan.framework.bn.BayesianNet`.
        :param observed: A dictionary of ``(string, Tensor)`` pairs: the observed nodes.
        :param latent: A dictionary of ``(string, Tensor)`` pairs: the current state of the chains.  The chain shape is that
            of ``bn.log_joint()``; every latent's shape begins with it.
        :param inplace: write the new state into the storage of the given tensors and return those objects.
        :return: ``(samples, info)``: a dict like ``latent`` and an :class:`HMCInfo` of device tensors.
        """
        names = list(latent.keys())
        given = [latent[k] for k in names]
        if not names:
            raise ValueError("HMC.sample: no latent given")
        for k, t in zip(names, given):
            if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.float64):
                raise ValueError("HMC.sample: latent '%s' must be a float32 or float64 tensor" % k)
            if inplace and not t.is_contiguous():
                raise ValueError("HMC.sample(inplace=True): latent '%s' is not contiguous" % k)
        q0 = [t.detach().contiguous() for t in given]
        device = q0[0].device

        logp0, grads = self._log_joint_and_grad(bn, observed, names, q0)
        chain_shape = tuple(logp0.shape)
        n_chains = int(logp0.numel())
        for k, t in zip(names, q0):
            if tuple(t.shape[:len(chain_shape)]) != chain_shape:
                raise ValueError("HMC.sample: latent '%s' has shape %s, which does not begin with the chain shape %s of the log "
                                 "joint" % (k, tuple(t.shape), chain_shape))
        logp0 = logp0.contiguous().view(-1)
        chunks = self._plan(names, q0, n_chains)
        state = self._state_on(device)

        # draws, in the order of the contract: the momenta per latent in latent order, then one [C] uniform
        z = [_rng.pop_injected(tuple(t.shape), device, t.dtype) for t in q0]
        u = _rng.pop_injected((n_chains,), device, logp0.dtype, kind="rand")
        seed, call, rng_state = _rng.next_call(device)

        q = [None] * len(q0)
        p0 = [None] * len(q0)
        work = []
        for j, c in enumerate(chunks):
            cq, cp, cp0 = [c.split(torch.empty(c.n, dtype=c.dtype, device=device)) for _ in range(3)]
            ksum = [torch.empty(n_chains * c.slots, dtype=c.dtype, device=device) for _ in range(2)]
            cz = [z[i] for i in c.idx]
            _hmc_hip.move(_hmc_hip.BEGIN, n_chains, state, cq, cp, [grads[i] for i in c.idx], q0=[q0[i] for i in c.idx],
                          z=None if all(e is None for e in cz) else cz, p0=cp0, ksum=ksum[0], seed=seed,
                          call=call + j * _CHUNK_CALL_STRIDE, rng_state=rng_state)
            for i, a, b in zip(c.idx, cq, cp0):
                q[i], p0[i] = a, b
            work.append((c, cq, cp, ksum))
        moved = [q[i] if q[i] is not None else q0[i] for i in range(len(q0))]      # (an empty latent stays where it is)
        logp1 = None
        for l in range(self.n_leapfrogs):
            logp1, grads = self._log_joint_and_grad(bn, observed, names, moved)
            last = l == self.n_leapfrogs - 1
            for c, cq, cp, ksum in work:
                _hmc_hip.move(_hmc_hip.END if last else _hmc_hip.STEP, n_chains, state, cq, cp, [grads[i] for i in c.idx],
                              ksum=ksum[1] if last else None)
        logp1 = logp1.contiguous().view(-1)

        out = torch.empty(5 * n_chains, dtype=torch.float64, device=device)
        accept = torch.empty(n_chains, dtype=torch.int32, device=device)
        seed, call, rng_state = _rng.next_call(device)
        _hmc_hip.decide([(ksum[0], ksum[1], c.slots) for c, _, _, ksum in work], n_chains, logp0, logp1, u, state, out, accept,
                        self.adapt_step_size, self.target_acceptance_rate, self.gamma, self.t0, self.kappa, seed=seed, call=call,
                        rng_state=rng_state)

        result = [t if inplace else torch.empty_like(a) for t, a in zip(given, q0)]
        for c, cq, _, _ in work:
            _hmc_hip.select(n_chains, [q0[i] for i in c.idx], cq, [result[i].detach() for i in c.idx], accept)
        for i, t in enumerate(q0):
            if not t.numel() and not inplace:
                result[i] = t.clone()
        self.t += 1

        samples = dict(zip(names, result))
        rows = out.view(5, n_chains).to(logp0.dtype)
        info = HMCInfo(samples=samples, acceptance_rate=rows[0].view(chain_shape), updated_step_size=state[_hmc_hip.EPS].clone(),
                       init_momentum=dict((k, m) for k, m in zip(names, p0) if m is not None),
                       orig_hamiltonian=rows[1].view(chain_shape), hamiltonian=rows[2].view(chain_shape),
                       orig_log_prob=logp0.view(chain_shape), log_prob=rows[4].view(chain_shape))
        return samples, info
