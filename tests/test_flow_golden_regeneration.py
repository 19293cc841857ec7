"""The committed flow fixtures (tests/golden/flow/) are exactly what tests/golden/flow/gen_flow_golden.py produces from the
real reference.  Build container only (skipped where the reference checkout is not present): the generator runs into a
temporary directory in a subprocess and every array of every fixture is compared bit for bit with the committed one."""
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN
from reference_runs import REF, same_fixtures

FLOW = os.path.join(GOLDEN, "flow")


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "zhusuan", "invertible")), reason="reference checkout not present")
def test_flow_goldens_regenerate_bit_identically(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(FLOW, "gen_flow_golden.py"), "--ref", REF, "--out", str(tmp_path)],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert same_fixtures(str(tmp_path), FLOW) > 300
    assert len([f for f in os.listdir(FLOW) if f.endswith(".npz")]) == 7
