"""The reference's OWN unittest files for this path, run unmodified against this package.

Only where the reference checkout exists (the build container); skipped elsewhere.  The files
(test/variational/test_elbo.py, test_iw.py, test/distributions/test_normal.py, test_bernoulli.py, test_logistic.py,
test_uniform.py, the six pass-through families' test files, test_base.py and their helper modules) are copied to a temporary directory at run time -- nothing of them is kept in this repository --
and executed in a subprocess whose `zhusuan` is THIS package with the CPU oracle library as kernel back-end
(tests/reference_runs.py, tests/ref_plugin.py).  They use CPU tensors, so this is the host-logic / drop-in check: same constructor
errors, shapes, dtypes (incl. float64), scipy known answers, analytic-KL gradient tests, vimco-vs-sgvb test.
"""
import os

import pytest

from reference_runs import REF, run_reference_tests

# the kernel-backed families, then the six torch.distributions wrapper families (off the hot path: plain pass-throughs here too)
# and the base class
FAMILIES = ["normal", "bernoulli", "logistic", "uniform", "beta", "exponential", "gamma", "laplace", "poisson", "studentT", "base"]


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "test")), reason="reference checkout not present")
def test_reference_unittests_pass_against_this_package(tmp_path):
    targets = ["variational"] + ["distributions/test_%s.py" % f for f in FAMILIES]
    files = ["__init__.py", "variational/__init__.py", "variational/utils.py", "variational/test_elbo.py", "variational/test_iw.py",
             "distributions/__init__.py", "distributions/utils.py"] + targets[1:]
    n_passed = run_reference_tests(tmp_path, files, targets, "", env={"MPLBACKEND": "Agg"})
    # 3 (elbo) + 3 (iw) + 11 (normal) + 7 (bernoulli) + 9 (logistic) + 9 (uniform) = 42 on the kernel-backed path,
    # + 48 for the six torch.distributions pass-through families and test_base.py
    assert n_passed >= 90
