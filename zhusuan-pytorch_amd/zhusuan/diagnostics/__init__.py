"""Convergence diagnostics of the samplers' output: split R-hat, effective sample size and autocorrelation of every element of a
stack of chains, each in one kernel launch (include/zs_diag.h; lib/libzs_diag.so, loaded on the first call).  Not imported by
``import zhusuan``, as with ``zhusuan.mcmc``.

``draws`` is a float32 or float64 tensor ``[T, *chains, *event]`` on the GPU: ``T`` draws, then ``chain_ndims`` axes that index
chains (``HMC``'s chain shape may have several), then the event.  A dict of such tensors gives a dict of results.  A view whose
event axes are contiguous -- a ``[C, T, ...]`` stack seen as ``[T, C, ...]``, a slice of draws -- runs as it is; any other layout
is made contiguous first.  Nothing here synchronises with the host.

The estimators are those defined in include/zs_diag.h (Gelman et al., BDA3; Vehtari et al. 2021, without rank normalisation)."""
import collections
import math

import torch

from .. import _diag_hip

__all__ = ["Summary", "summary", "ess", "rhat", "autocorrelation", "effective_sample_size", "Trace"]

Summary = collections.namedtuple("Summary", "mean var rhat ess lags capped")
Summary.__doc__ = """Per element of the event: ``mean`` over all chains, ``var`` (the estimate var+ of the marginal posterior
variance), ``rhat``, ``ess``, ``lags`` (int32: the autocorrelation lags that entered ``ess``) and ``capped`` (int32: 1 where the
lag loop ended at ``max_lag`` or at the chain's length rather than on a non-positive pair)."""


def _collapse(sizes, strides):
    """The one stride that walks the row-major product of ``sizes``, or None when there is none; 0 for a product of 1."""
    stride = None
    for n, s in reversed(list(zip(sizes, strides))):
        if n == 1:
            continue
        if stride is None:
            stride, span = s, s * n
        elif s == span:
            span = s * n
        else:
            return None
    return 0 if stride is None else stride


def _operand(draws, chain_ndims, who):
    """(x, st, sc, T, C, E, chain shape, event shape): ``draws`` as the kernel addresses it, copied only if it must be."""
    if not isinstance(draws, torch.Tensor):
        raise TypeError("zhusuan.diagnostics.%s: draws must be a tensor or a dict of tensors, got %s" % (who, type(draws).__name__))
    if draws.dtype not in (torch.float32, torch.float64):
        raise TypeError("zhusuan.diagnostics.%s: draws must be float32 or float64, got %s" % (who, draws.dtype))
    chain_ndims = int(chain_ndims)
    if chain_ndims < 0 or draws.dim() < 1 + chain_ndims:
        raise ValueError("zhusuan.diagnostics.%s: draws of shape %s have no %d chain axes after the first" % (who, tuple(draws.shape), chain_ndims))
    draws = draws.detach()
    T = draws.shape[0]
    chains, event = tuple(draws.shape[1:1 + chain_ndims]), tuple(draws.shape[1 + chain_ndims:])
    C, E = int(math.prod(chains)), int(math.prod(event))
    strides = draws.stride()
    sc = _collapse(chains, strides[1:1 + chain_ndims])
    se = _collapse(event, strides[1 + chain_ndims:])
    st = strides[0] if T > 1 else 0
    ok = sc is not None and se == (1 if E > 1 else 0)          # (a stride of 0 over E > 1 elements is an expanded axis: copied)
    if ok and T > 1 and C > 1:          # the two outer strides step over what lies inside them
        ok = (sc >= E and st >= sc * C) if st >= sc else (st >= E and sc >= st * T)
    elif ok and (T > 1 or C > 1):
        ok = max(st, sc) >= E
    if not ok:
        draws = draws.contiguous()
        st, sc = C * E, E
    return draws, st, (sc if C > 1 else E), T, C, E, chains, event


def _summary(draws, chain_ndims, split, max_lag, want, who):
    if isinstance(draws, dict):
        return {k: _summary(v, chain_ndims, split, max_lag, want, who) for k, v in draws.items()}
    x, st, sc, T, C, E, chains, event = _operand(draws, chain_ndims, who)
    N = T // 2 if split else T
    if N < 2:
        raise ValueError("zhusuan.diagnostics.%s: %d draws of %d chains%s leave chains of length %d; at least 2 are needed"
                         % (who, T, C, " (split)" if split else "", N))
    if C < 1:
        raise ValueError("zhusuan.diagnostics.%s: draws of shape %s hold no chain" % (who, tuple(draws.shape)))
    if E == 0:
        outs = [None if n not in want else x.new_empty(0, dtype=torch.int32 if n in ("lags", "capped") else x.dtype)
                for n in _diag_hip.OUTPUTS]
    else:
        outs = _diag_hip.summary(x, st, sc, T, C, E, bool(split), -1 if max_lag is None else int(max_lag), want)
    return Summary(*[None if o is None else o.view(event) for o in outs])


def summary(draws, chain_ndims=0, split=True, max_lag=None):
    """``Summary(mean, var, rhat, ess, lags, capped)`` of ``draws`` ``[T, *chains, *event]``, every field of the event shape.
    ``split``: every chain enters as its two halves (an odd ``T`` drops the middle draw).  ``max_lag``: the largest
    autocorrelation lag the effective sample size may use (None: the chain's length decides)."""
    if max_lag is not None and int(max_lag) < 0:
        raise ValueError("zhusuan.diagnostics.summary: max_lag must be None or >= 0, got %s" % (max_lag,))
    return _summary(draws, chain_ndims, split, max_lag, _diag_hip.OUTPUTS, "summary")


def _field(result, name):
    return {k: getattr(v, name) for k, v in result.items()} if isinstance(result, dict) else getattr(result, name)


def ess(draws, chain_ndims=0, split=True, max_lag=None):
    """The effective sample size per element (the ``ess`` of ``summary``, alone)."""
    if max_lag is not None and int(max_lag) < 0:
        raise ValueError("zhusuan.diagnostics.ess: max_lag must be None or >= 0, got %s" % (max_lag,))
    return _field(_summary(draws, chain_ndims, split, max_lag, ("ess",), "ess"), "ess")


def rhat(draws, chain_ndims=0, split=True):
    """The potential scale reduction per element (the ``rhat`` of ``summary``, alone: the lag loop does not run)."""
    return _field(_summary(draws, chain_ndims, split, None, ("rhat",), "rhat"), "rhat")


def autocorrelation(draws, max_lag, chain_ndims=0):
    """The autocorrelation of every chain at lags ``0 .. max_lag``: ``[max_lag + 1, *chains, *event]`` (the curve one plots)."""
    if isinstance(draws, dict):
        return {k: autocorrelation(v, max_lag, chain_ndims) for k, v in draws.items()}
    x, st, sc, T, C, E, chains, event = _operand(draws, chain_ndims, "autocorrelation")
    L = int(max_lag)
    if L < 0 or L > T - 1:
        raise ValueError("zhusuan.diagnostics.autocorrelation: max_lag must lie in [0, T - 1] = [0, %d], got %d" % (T - 1, L))
    if C * E == 0:
        return x.new_empty((L + 1,) + chains + event)
    return _diag_hip.autocorr(x, st, sc, T, C, E, L).view((L + 1,) + chains + event)


def effective_sample_size(samples, burn_in=100):
    """ZhuSuan's ``zhusuan.diagnostics.effective_sample_size(samples, burn_in=100)``: drops the first ``burn_in`` draws of
    ``samples`` ``[T, ...]``, treats the rest as ONE unsplit chain and returns the smallest effective sample size over all
    elements, a 0-dim tensor.  The estimator is the one defined in include/zs_diag.h (Geyer's initial monotone sequence); it
    carries upstream's name and arguments and does not claim to reproduce upstream's numbers bit for bit."""
    burn_in = int(burn_in)
    if burn_in < 0:
        raise ValueError("zhusuan.diagnostics.effective_sample_size: burn_in must be >= 0, got %d" % burn_in)
    if not isinstance(samples, torch.Tensor):
        raise TypeError("zhusuan.diagnostics.effective_sample_size: samples must be a tensor, got %s" % type(samples).__name__)
    return ess(samples[burn_in:], chain_ndims=0, split=False).min()


class Trace(object):
    """The draws of a sampling run, kept on the device::

        trace = Trace(n_draws)
        for i in range(n_draws):
            latent, info = sampler.sample(model, observed, latent)          # or: latent = sgmcmc.sample(model, observed)
            trace.append(latent)
        print(trace.summary(chain_ndims=1))

    ``append`` copies every tensor of the dict (or of the dict that leads a tuple, as ``HMC.sample`` returns) into row ``i`` of a
    buffer ``[n_draws, *shape]`` that the first append allocates; the copy is enqueued on the current stream and does not
    synchronise."""

    def __init__(self, n_draws):
        n_draws = int(n_draws)
        if n_draws < 1:
            raise ValueError("zhusuan.diagnostics.Trace: n_draws must be >= 1, got %d" % n_draws)
        self.n_draws = n_draws
        self._buffers = None
        self._filled = 0

    def __len__(self):
        return self._filled

    def append(self, latent):
        if isinstance(latent, tuple) and latent and isinstance(latent[0], dict):
            latent = latent[0]
        if not isinstance(latent, dict):
            raise TypeError("zhusuan.diagnostics.Trace.append: expected a dict of name -> tensor, got %s" % type(latent).__name__)
        if self._filled >= self.n_draws:
            raise IndexError("zhusuan.diagnostics.Trace.append: the trace already holds its %d draws" % self.n_draws)
        if self._buffers is None:
            self._buffers = {k: torch.empty((self.n_draws,) + tuple(v.shape), dtype=v.dtype, device=v.device) for k, v in latent.items()}
        if set(latent) != set(self._buffers):
            raise KeyError("zhusuan.diagnostics.Trace.append: latents %s differ from the first draw's %s" % (sorted(latent), sorted(self._buffers)))
        for k, v in latent.items():
            self._buffers[k][self._filled].copy_(v.detach(), non_blocking=True)
        self._filled += 1

    @property
    def draws(self):
        """name -> the filled prefix ``[len(self), *shape]`` (a view of the buffer)."""
        return {} if self._buffers is None else {k: b[:self._filled] for k, b in self._buffers.items()}

    def summary(self, chain_ndims=0, split=True, max_lag=None):
        """name -> ``Summary`` of the draws so far: one launch per latent."""
        return summary(self.draws, chain_ndims=chain_ndims, split=split, max_lag=max_lag)
