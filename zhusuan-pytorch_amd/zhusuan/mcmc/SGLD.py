"""SGLD and PSGLD.  Interface of zhusuan/mcmc/SGLD.py:8-82 of the reference; per step one ``autograd.grad`` of the log
joint and ONE fused launch over all latents of a dtype (ZS_MCMC_SGLD / ZS_MCMC_PSGLD of include/zs_mcmc.h)."""
from .. import _mcmc_hip
from .SGMCMC import SGMCMC

# (the reference's module has no __all__: its star-import also hands on the base class)
__all__ = ["SGLD", "PSGLD", "SGMCMC"]


class SGLD(SGMCMC):
    """
    Stochastic Gradient Langevin Dynamics (Welling & Teh, 2011), Equation (3) of the paper:
    ``q' = q + (lr/2) grad log p(q) + N(0, lr)`` (SGLD.py:50-52).

    :param learning_rate: A Python number or 0-D tensor.
    """

    def __init__(self, learning_rate):
        super().__init__()
        self.lr = float(learning_rate)

    def _update(self, bn, observed):
        grads = self._log_joint_grads(bn, observed)
        for chunk in self._chunks:
            self._launch(_mcmc_hip.SGLD, chunk, grads, z=self._draws(chunk), use_state=False, lr=self.lr)


class PSGLD(SGLD):
    """
    PSGLD with RMSprop preconditioner, "Preconditioned stochastic gradient Langevin dynamics for deep neural networks"
    (SGLD.py:67-82): ``a' = decay a + (1 - decay) g^2``, ``G = 1 / (epsilon + sqrt(a'))``,
    ``q' = q + (lr/2) G g + N(0, lr G)``.  ``a`` is one flat device buffer per launch, updated in place.
    """

    def __init__(self, learning_rate, decay=0.9, epsilon=1e-3):
        super().__init__(learning_rate)
        self.decay = decay
        self.epsilon = epsilon

    @property
    def aux(self):
        """The running second moments, per latent (views of the flat state), or None before the first update."""
        if not self._chunks or any(c.state is None for c in self._chunks):
            return None
        out = {}
        for c in self._chunks:
            out.update(zip(c.idx, c.split(c.state)))
        return [out[i] for i in sorted(out)]

    def _update(self, bn, observed):
        grads = self._log_joint_grads(bn, observed)
        for chunk in self._chunks:
            self._launch(_mcmc_hip.PSGLD, chunk, grads, z=self._draws(chunk), lr=self.lr, decay=self.decay,
                         epsilon=self.epsilon)
