"""Base class of the stochastic-gradient MCMC samplers.  Interface of zhusuan/mcmc/SGMCMC.py:9-76 of the reference;
the update itself is one fused launch over all latents (csrc/zs_mcmc.hip, include/zs_mcmc.h)."""
import torch
import torch.nn as nn

from .. import _mcmc_hip, _rng
from ._chunks import Chunk, plan_chunks

__all__ = [
    "SGMCMC"
]


class _Chunk(Chunk):
    """The latents of one launch: at most _mcmc_hip.MAX_TENSORS tensors of one dtype, forming one flat index space."""

    def __init__(self, idx, shapes, dtype, device):
        super().__init__(idx, shapes, dtype)
        self.device = device
        self.state = None          # flat, device-resident (PSGLD's second moment, SGHMC's velocity)

    def key(self):
        return (tuple(self.idx), tuple(tuple(s) for s in self.shapes), self.dtype, self.device)


class SGMCMC(nn.Module):
    """
    Base class for stochastic gradient MCMC (SGMCMC) algorithms: SGLD, PSGLD, SGHMC.

    The typical code for SGMCMC inference is like::

        sgmcmc = zs.mcmc.SGLD(learning_rate=lr)
        net = BayesianNet()
        w_samples = sgmcmc.sample(net, {'x': x, 'y': y}, resample=True)
        for step in range(num_steps):
            w_samples = sgmcmc.sample(net, {'x': x, 'y': y})
    """

    def __init__(self):
        super().__init__()
        self.t = 0
        self._device = torch.device('cpu')      # SGLD.py:22: the reference's default; the updates run where the latents live
        self._chunks = []

    @property
    def device(self):
        """The device given to ``to`` (SGLD.py:24-38), or that of the latents once there are some."""
        return self._device

    def to(self, device):
        self._device = torch.device(device) if not isinstance(device, torch.device) else device
        return super().to(device)

    # ------------------------------------------------------------------------------------------------ the fused launch
    def _plan(self):
        """Group the latents into launches; the state of a group survives a resample that keeps its layout (the reference
        keeps ``aux`` / ``vs`` across ``resample=True``, SGLD.py:68-69, SGHMC.py:26-27)."""
        old = dict((c.key(), c) for c in self._chunks)
        chunks = []
        for (dtype, device), part in plan_chunks(self._var_list, lambda q: (q.dtype, q.device), _mcmc_hip.MAX_TENSORS):
            c = _Chunk(part, [self._var_list[i].shape for i in part], dtype, device)
            chunks.append(old.get(c.key(), c))
        self._chunks = chunks

    def _draws(self, chunk):
        """The standard normals of one draw per latent of `chunk`, asked for in latent order: injected tensors
        (``zhusuan.inject_epsilon``), host draws (``zhusuan.reference_rng``), or None: the kernel draws."""
        zs = [_rng.pop_injected(tuple(s), chunk.device, chunk.dtype) for s in chunk.shapes]
        return None if all(z is None for z in zs) else zs

    def _launch(self, kind, chunk, grads=None, z=None, new_q=True, use_state=True, flags=0, call=None, **hyper):
        """One fused update of the latents of `chunk`; returns nothing, replaces their entries of ``_var_list`` by new
        detached leaves that require grad (``q_out != q_in``: a caller that kept the previous values keeps them)."""
        q_in = [self._var_list[i].detach().contiguous() for i in chunk.idx]
        if new_q:
            q_out = chunk.split(torch.empty(chunk.n, dtype=chunk.dtype, device=chunk.device))
        else:
            q_out = q_in
        state = None
        if use_state:
            if chunk.state is None:
                chunk.state = torch.zeros(chunk.n, dtype=chunk.dtype, device=chunk.device)
            state = chunk.split(chunk.state)
        if grads is not None:
            grads = [grads[i].detach().contiguous() for i in chunk.idx]
        seed, call_id, rng_state = call if call is not None else _rng.next_call(chunk.device)
        _mcmc_hip.update(kind, q_in, q_out, grad=grads, state=state, z=z, flags=flags, seed=seed, call=call_id,
                         rng_state=rng_state, **hyper)
        if new_q:
            for i, q in zip(chunk.idx, q_out):
                self._var_list[i] = q.requires_grad_(True)

    def _log_joint_grads(self, bn, observed):
        """The gradient of the log joint at the current latents: one forward with the latents observed, one
        ``autograd.grad`` through the existing kernels (SGLD.py:43-48)."""
        observed_ = {**dict(zip(self._latent_k, self._var_list)), **observed}
        bn.forward(observed_)
        log_joint_ = bn.log_joint()
        return torch.autograd.grad(log_joint_, self._var_list)

    def _update(self, bn, observed):
        raise NotImplementedError()

    # ------------------------------------------------------------------------------------------------ SGMCMC.py:38-59
    def forward(self, bn, observed, resample=False, step=1):
        if resample:
            self.t = 0
            bn.forward(observed)
            self.t += 1

            self._latent = {k: v.tensor for k, v in bn.nodes.items() if k not in observed.keys()}
            self._latent_k = list(self._latent.keys())
            self._var_list = [self._latent[k] for k in self._latent_k]
            sample_ = dict(zip(self._latent_k, self._var_list))

            for i in range(len(self._var_list)):
                self._var_list[i] = self._var_list[i].detach()
                self._var_list[i].requires_grad = True
            if self._var_list:
                self._device = self._var_list[0].device
            self._plan()
            return sample_

        for s in range(step):
            self._update(bn, observed)
            self.t += 1

        sample_ = dict(zip(self._latent_k, self._var_list))
        return sample_

    def initialize(self):
        self.t = 0

    def sample(self, bn, observed, resample=False, step=1):
        """
        Running sgmcmc iterations.

        :param bn: A instance of :class:`~zhusuan.framework.bn.BayesianNet`.
        :param observed: A dictionary of ``(string, Tensor)`` pairs. Mapping from names of
            observed `StochasticTensor` s to their values.
        :param resample: Flag indicates if the sampler need get the var list of
            the :class:`~zhusuan.framework.bn.BayesianNet` instance, usually set to True on first sgmcmc iteration.
        :param step: number of updates made by this call.
        :return: A dict of latent name -> sample generated by the last iteration.
        """
        return self.forward(bn, observed, resample, step)
