"""The reference's OWN flow tests (test/invertible/test_invertible.py), run unmodified against this package.

Only where the reference checkout exists; skipped elsewhere.  The file is copied to a temporary directory at run time --
nothing of it is kept in this repository -- and its eleven tests (construction of every layer, the three mask types, and
``forward`` then ``reverse=True`` recovering a [1, 200] input to 1e-4 in summed absolute error for Scaling, Coupling,
MaskCoupling, a RevSequential of four couplings and MADE) run in a subprocess whose `zhusuan` is THIS package on the host
back-end (tests/reference_runs.py, suite "flow" of tests/ref_plugin.py), with a fixed seed."""
import os

import pytest

from reference_runs import REF, run_reference_tests


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "test", "invertible", "test_invertible.py")),
                    reason="reference checkout not present")
def test_reference_flow_tests_pass_against_this_package(tmp_path):
    n_passed = run_reference_tests(tmp_path, ["__init__.py", "invertible/__init__.py", "invertible/test_invertible.py"],
                                   ["invertible/test_invertible.py"], "flow", env={"ZS_FLOW_SUITE_SEED": "0"}, timeout=600)
    assert n_passed == 11
