"""examples/hmc_diagnostics.py -- HMC chains into a ``Trace``, the summary in one launch -- at a tiny size on both back-ends.  Only
what holds by construction is asserted; the figures it prints at the default seed are recorded in tests/README_diag.md."""
import math

import torch

import diag_host
import hmc_host
import host_backend
import host_routing

xdev = host_routing.dev_fixture("xdev", hmc_host.router, diag_host.router)


def test_example_runs_at_a_tiny_size(xdev):
    from examples import hmc_diagnostics
    host_backend.manual_seed(1)
    n_x, n_chains, n_iters = 2, 4, 60
    with diag_host.router.count() as launches:
        r = hmc_diagnostics.run(n_x=n_x, n_chains=n_chains, n_iters=n_iters, n_leapfrogs=3, device=xdev)
    assert launches["summary"] == 1 and launches["autocorr"] == 0
    lines = []
    hmc_diagnostics.report(r, log=lines.append)
    print("\n".join(lines))
    draws = r["trace"].draws["x"]
    assert len(r["trace"]) == n_iters // 2 and tuple(draws.shape) == (n_iters // 2, n_chains, n_x) and draws.device == xdev
    s = r["summary"]
    for name in ("mean", "var", "rhat", "ess"):
        t = getattr(s, name)
        assert tuple(t.shape) == (n_x,) and t.dtype == torch.float32 and t.device == xdev and bool(torch.isfinite(t).all()), name
    assert s.lags.dtype == torch.int32 and s.capped.dtype == torch.int32 and tuple(s.lags.shape) == (n_x,)
    # by construction: M = 2 * 4 split chains of N = 15 draws
    M, N = 2 * n_chains, n_iters // 4
    assert bool((s.ess > 0).all()) and bool((s.ess.double() <= M * N * math.log10(M * N) * (1 + 2.0 ** -22)).all())
    assert bool((s.var > 0).all()) and bool((s.rhat > 0).all())
    assert bool((s.lags >= 0).all()) and bool((s.lags <= N).all()) and bool((s.lags % 2 == 0).all())
    assert len(lines) == 1 + n_x
