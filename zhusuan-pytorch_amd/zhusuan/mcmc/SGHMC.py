"""SGHMC.  Interface of zhusuan/mcmc/SGHMC.py:12-56 of the reference; per step one ``autograd.grad`` of the log joint, one
fused launch after it (ZS_MCMC_SGHMC_POST of include/zs_mcmc.h) and, when ``second_order`` or a velocity resample is due, one
before it (ZS_MCMC_SGHMC_PRE)."""
from .. import _mcmc_hip, _rng
from .SGMCMC import SGMCMC

__all__ = [
    "SGHMC",
]


class SGHMC(SGMCMC):
    """
    Stochastic Gradient Hamiltonian Monte Carlo (Chen et al., 2014).

    :param learning_rate: step size.
    :param friction: ``alpha``.
    :param variance_estimate: ``beta``, the estimate of the gradient noise; at most ``friction``.
    :param n_iter_resample_v: the velocities are redrawn from N(0, lr) whenever ``t`` is a multiple of it (None or 0: never).
    :param second_order: the symmetric splitting: half a position step before the gradient and half after it.
    """

    def __init__(self, learning_rate, friction=0.25, variance_estimate=0.,
                 n_iter_resample_v=20, second_order=True):
        super(SGHMC, self).__init__()
        self.lr = learning_rate
        self.alpha = friction
        self.beta = variance_estimate
        if n_iter_resample_v is None:
            n_iter_resample_v = 0
        self.n_iter_resample_v = n_iter_resample_v
        self.second_order = second_order

    @property
    def vs(self):
        """The velocities, per latent (views of the flat state), or None before the first update.
        Deviation from the reference: they live on the latents' device (and so does the noise); the reference draws both on
        the host and leaves them there (SGHMC.py:27,33-34), which fails for latents on a GPU."""
        if not self._chunks or any(c.state is None for c in self._chunks):
            return None
        out = {}
        for c in self._chunks:
            out.update(zip(c.idx, c.split(c.state)))
        return [out[i] for i in sorted(out)]

    def _update(self, bn, observed):
        order = _mcmc_hip.SECOND_ORDER if self.second_order else 0
        due = self.n_iter_resample_v != 0 and self.t % self.n_iter_resample_v == 0
        # The reference's draws, in its order (SGHMC.py:26-34): the initial velocities of ALL latents on the first update, then
        # latent by latent a redrawn velocity (when due; on the first update it overwrites the initial one, which was drawn
        # all the same) and the gaussian term.  Injected / host draws are popped in exactly that order; on the Philox path a
        # draw is a call id, consumed also where its values are never used.
        first = [c.state is None for c in self._chunks]
        pre_z, pre_call, post_z = [], [], []
        for c, f in zip(self._chunks, first):
            pre_z.append(self._draws(c) if f else None)
            pre_call.append(_rng.next_call(c.device) if f and pre_z[-1] is None else None)
        for k, c in enumerate(self._chunks):
            zr, zg = [], []
            for j, s in enumerate(c.shapes):
                if due:
                    zr.append(_rng.pop_injected(tuple(s), c.device, c.dtype))
                zg.append(_rng.pop_injected(tuple(s), c.device, c.dtype))
            if due:
                if all(z is None for z in zr):
                    pre_z[k], pre_call[k] = None, _rng.next_call(c.device)
                else:
                    pre_z[k] = zr
            # Deviation from the reference: every latent gets its OWN gaussian term.  The reference's loop keeps only the last
            # latent's draw and adds it to all of them (SGHMC.py:29-34,47,53), which works only where the shapes broadcast;
            # the number and order of draws are the reference's.
            post_z.append(None if all(z is None for z in zg) else zg)
        for k, c in enumerate(self._chunks):
            draw = first[k] or due
            if draw or self.second_order:
                self._launch(_mcmc_hip.SGHMC_PRE, c, z=pre_z[k] if draw else None, new_q=bool(self.second_order),
                             flags=order | (_mcmc_hip.RESAMPLE_V if draw else 0), call=pre_call[k] if draw else (0, 0, None),
                             lr=self.lr)
        grads = self._log_joint_grads(bn, observed)
        for k, c in enumerate(self._chunks):
            self._launch(_mcmc_hip.SGHMC_POST, c, grads, z=post_z[k], flags=order, lr=self.lr, alpha=self.alpha, beta=self.beta)
