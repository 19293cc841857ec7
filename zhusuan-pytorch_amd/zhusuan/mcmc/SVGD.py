"""Stein variational gradient descent (Liu & Wang 2016): a set of K interacting particles moved along the kernelised gradient.

The reference (thuwzy/ZhuSuan-PyTorch) has no particle method.  The calling convention is ``HMC.sample``'s: the particle shape is
that of ``bn.log_joint()``, every latent's shape begins with it, one forward and one ``autograd.grad`` through the existing kernels
per step.  On a HIP device with K up to the kernels' cap (256 particles for float32, 128 for float64) a step is, per chunk of
latents, three launches of lib/libzs_svgd.so (csrc/zs_svgd.hip, include/zs_svgd.h): gram, finish, update -- with several chunks
(mixed dtypes, more than 32 latents) every chunk's gram, ONE finish over all partials, every chunk's update.  CPU tensors and
wider particle sets run ``torch_step``, a torch composition of the same formulas; ``last_path`` says which path ran and why.
Nothing here synchronises the host."""
import collections
import math

import torch

from .. import _svgd_hip
from ._chunks import Chunk, plan_chunks
from .HMC import HMC

__all__ = [
    "SVGD", "SVGDInfo"
]

SVGDInfo = collections.namedtuple("SVGDInfo", ["bandwidth", "kernel", "log_prob"])


def torch_step(thetas, grads, bandwidth=None):
    """The formulas of include/zs_svgd.h in torch, on any device: ``thetas`` and ``grads`` are lists of [K, M_t] tensors (dtypes
    may differ between entries).  The Gram matrix of the column-centred particles is formed per tensor in that tensor's dtype and
    summed, like everything after it, in float64 -- what the kernels do.  Returns (phis, kernel [K, K] float64, h [] float64)."""
    K = thetas[0].shape[0]
    centred = [t - t.mean(0, keepdim=True) for t in thetas]
    G = sum((c @ c.t()).double() for c in centred)
    diag = torch.diagonal(G)
    d = (diag[:, None] + diag[None, :] - 2.0 * G).clamp_min(0.0)
    d = d - torch.diag_embed(torch.diagonal(d))
    d = 0.5 * (d + d.t())
    if bandwidth is None:
        med = torch.quantile(d.reshape(-1), 0.5)          # the mean of the two middle values of an even count
        h = torch.where(med > 0, med / math.log(K + 1.0), torch.ones_like(med))
    else:
        h = torch.tensor(float(bandwidth), dtype=torch.float64, device=d.device)
    kernel = torch.exp(-d / h)
    s = kernel.sum(1)
    phis = []
    for c, g in zip(centred, grads):
        k, two_h = kernel.to(c.dtype), (2.0 / h).to(c.dtype)
        phis.append((k @ (g - two_h * c) + two_h * s.to(c.dtype)[:, None] * c) / K)
    return phis, kernel, h


def precondition(phi, H, first, alpha, fudge):
    """The authors' AdaGrad with momentum: the new second moment and the preconditioned direction."""
    H = phi * phi if first else alpha * H + (1.0 - alpha) * (phi * phi)
    return H, phi / (fudge + torch.sqrt(H))


class _Chunk(Chunk):
    """The latents of one launch: at most _svgd_hip.MAX_TENSORS tensors of one dtype, forming one flat column space."""

    def __init__(self, idx, shapes, dtype, n_particles):
        super().__init__(idx, shapes, dtype)
        self.slots = _svgd_hip.slots(self.n // n_particles)
        self.state = None          # flat, device-resident: AdaGrad's second moment


class SVGD(object):
    """
    Stein variational gradient descent with the RBF kernel::

        svgd = zs.mcmc.SVGD(step_size=1e-3)
        latent = {'w': w0}                                # [K, ...]: K particles
        for it in range(n_iters):
            latent, info = svgd.sample(net, {'x': x, 'y': y}, latent)

    :param step_size: the step along phi.
    :param bandwidth: h of k(x, y) = exp(-|x - y|^2 / h); None is the median rule h = med / log(K + 1), med the median of all
        K^2 squared distances (h = 1 when it is 0).
    :param adagrad: precondition phi as the authors' code does: H = phi^2 on the first step after construction or
        ``initialize()``, then alpha H + (1 - alpha) phi^2; the step is step_size phi / (fudge + sqrt(H)).
    :param alpha, fudge: parameters of the preconditioner.
    """

    def __init__(self, step_size=1e-3, bandwidth=None, adagrad=False, alpha=0.9, fudge=1e-6):
        if not step_size > 0:
            raise ValueError("step_size must be positive")
        if bandwidth is not None and not float(bandwidth) > 0:
            raise ValueError("bandwidth must be positive, or None for the median rule")
        if not 0 <= alpha < 1:
            raise ValueError("alpha must be in [0, 1)")
        if not fudge > 0:
            raise ValueError("fudge must be positive")
        self.step_size = float(step_size)
        self.bandwidth = None if bandwidth is None else float(bandwidth)
        self.adagrad = bool(adagrad)
        self.alpha = float(alpha)
        self.fudge = float(fudge)
        self.t = 0
        self.last_path = None          # {"path": ..., "why": ...} of the last step
        self._first = True
        self._plan_key = None
        self._chunks = []
        self._host_state = None          # the torch path's second moments, one per latent

    def initialize(self):
        self.t = 0
        self._first = True

    # ------------------------------------------------------------------------------------------------ pieces of a step
    def _plan(self, names, qs, K):
        key = (tuple(names), tuple(tuple(q.shape) for q in qs), tuple(q.dtype for q in qs), qs[0].device, K)
        if key != self._plan_key:
            self._chunks = [_Chunk(part, [qs[i].shape for i in part], dtype, K)
                            for dtype, part in plan_chunks(qs, lambda q: q.dtype, _svgd_hip.MAX_TENSORS)]
            self._plan_key, self._host_state, self._first = key, None, True
        return self._chunks

    def _route(self, qs, K):
        if any(q.device.type != "cuda" for q in qs):
            return "CPU tensors"
        for q in qs:
            cap = _svgd_hip.MAX_PARTICLES[q.element_size()]
            if q.numel() and K > cap:
                return "K = %d particles, the %s kernels hold %d" % (K, str(q.dtype).replace("torch.", ""), cap)
        return None

    def _fused(self, chunks, K, q0, grads, result):
        device = q0[0].device
        partials = torch.empty(sum(c.slots for c in chunks) * K * K, dtype=torch.float64, device=device)
        state = torch.empty(_svgd_hip.state_doubles(K), dtype=torch.float64, device=device)
        at = 0
        for c in chunks:
            _svgd_hip.gram(K, [q0[i] for i in c.idx], partials[at * K * K:])
            at += c.slots
        _svgd_hip.finish(K, partials, at, state, self.bandwidth)
        for c in chunks:
            h = None
            if self.adagrad:
                if c.state is None:
                    c.state = torch.zeros(c.n, dtype=c.dtype, device=device)
                h = c.split(c.state)
            _svgd_hip.update(K, [q0[i] for i in c.idx], [grads[i] for i in c.idx], [result[i].detach() for i in c.idx], state,
                             self.step_size, h=h, first=self._first, alpha=self.alpha, fudge=self.fudge)
        return state[0], state[_svgd_hip.STATE_HEADER + K:].view(K, K)

    def _composed(self, K, q0, grads, result):
        live = [i for i, q in enumerate(q0) if q.numel()]
        phis, kernel, h = torch_step([q0[i].reshape(K, -1) for i in live], [grads[i].reshape(K, -1) for i in live], self.bandwidth)
        if self.adagrad and self._host_state is None:
            self._host_state = [None] * len(q0)
        for i, phi in zip(live, phis):
            if self.adagrad:
                self._host_state[i], phi = precondition(phi, self._host_state[i], self._first, self.alpha, self.fudge)
            result[i].detach().copy_((q0[i].reshape(K, -1) + self.step_size * phi).view(q0[i].shape))
        return h, kernel

    # ------------------------------------------------------------------------------------------------ one step
    def sample(self, bn, observed, latent, inplace=False):
        """
        One SVGD step.

        :param bn: A instance of :class:`~zhusuan.framework.bn.BayesianNet`.
        :param observed: A dictionary of ``(string, Tensor)`` pairs: the observed nodes.
        :param latent: A dictionary of ``(string, Tensor)`` pairs: the current particles.  The particle shape is that of
            ``bn.log_joint()``; every latent's shape begins with it.
        :param inplace: write the new particles into the storage of the given tensors and return those objects.
        :return: ``(samples, info)``: a dict like ``latent`` and an :class:`SVGDInfo` of device tensors -- the bandwidth h [],
            the kernel matrix [K, K] (float64) and the log joint of the particles the step started from.
        """
        names = list(latent.keys())
        given = [latent[k] for k in names]
        if not names:
            raise ValueError("SVGD.sample: no latent given")
        for k, t in zip(names, given):
            if not isinstance(t, torch.Tensor) or t.dtype not in (torch.float32, torch.float64):
                raise ValueError("SVGD.sample: latent '%s' must be a float32 or float64 tensor" % k)
            if inplace and not t.is_contiguous():
                raise ValueError("SVGD.sample(inplace=True): latent '%s' is not contiguous" % k)
        q0 = [t.detach().contiguous() for t in given]
        logp, grads = HMC._log_joint_and_grad(bn, observed, names, q0)
        shape = tuple(logp.shape)
        K = int(logp.numel())
        for k, t in zip(names, q0):
            if tuple(t.shape[:len(shape)]) != shape:
                raise ValueError("SVGD.sample: latent '%s' has shape %s, which does not begin with the particle shape %s of the "
                                 "log joint" % (k, tuple(t.shape), shape))
        if K < 1 or not any(t.numel() for t in q0):
            raise ValueError("SVGD.sample: there is nothing to move (no particle, or only empty latents)")
        result = [t if inplace else torch.empty_like(a) for t, a in zip(given, q0)]
        chunks = self._plan(names, q0, K)
        why = self._route(q0, K)
        if why is None:
            h, kernel = self._fused(chunks, K, q0, grads, result)
            self.last_path = {"path": "S1-S3 zs_svgd_gram, zs_svgd_finish, zs_svgd_update (%d chunk%s)"
                              % (len(chunks), "" if len(chunks) == 1 else "s"), "why": None}
        else:
            h, kernel = self._composed(K, q0, grads, result)
            self.last_path = {"path": "torch composition", "why": why}
        self._first = False
        self.t += 1
        return dict(zip(names, result)), SVGDInfo(bandwidth=h, kernel=kernel, log_prob=logp)
