"""The reference's OWN sampler tests (test/mcmc/test_mcmc.py), run unmodified against this package.

Only where the reference checkout exists; skipped elsewhere.  The file is copied to a temporary directory at run time --
nothing of it is kept in this repository -- and its four tests (SGLD, PSGLD, SGHMC first and second order: 8 000 steps of 100
chains on a double-well density with a noisy gradient, kernel-density estimate against the true density) run in a
subprocess whose `zhusuan` is THIS package on the host back-end (tests/reference_runs.py, suite "mcmc" of tests/ref_plugin.py),
with fixed seeds.  The thresholds are the reference's own: 0.023, 0.088, 0.016 and 0.016.  The reference alone reaches
0.014-0.018 (sgld), 0.074-0.076 (psgld) and 0.008-0.012 (sghmc) for seeds 0, 1, 2.
This package (seed 0, host back-end; deterministic): sgld 0.0140, psgld 0.0715, sghmc 0.0118, sghmc second order 0.0135."""
import os

import pytest

from reference_runs import REF, run_reference_tests


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "test", "mcmc", "test_mcmc.py")), reason="reference checkout not present")
def test_reference_sampler_tests_pass_against_this_package(tmp_path):
    n_passed = run_reference_tests(tmp_path, ["__init__.py", "mcmc/__init__.py", "mcmc/test_mcmc.py"], ["mcmc/test_mcmc.py"],
                                   "mcmc", env={"ZS_MCMC_SUITE_SEED": "0"})
    assert n_passed == 4
