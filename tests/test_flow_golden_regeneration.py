"""The committed flow fixtures (tests/golden/flow/) are exactly what tests/golden/flow/gen_flow_golden.py produces from the
real reference.  Build container only (skipped where the reference checkout is not present): the generator runs into a
temporary directory in a subprocess and every array of every fixture is compared bit for bit with the committed one."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN

REF = "/root/reference"
FLOW = os.path.join(GOLDEN, "flow")


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "zhusuan", "invertible")), reason="reference checkout not present")
def test_flow_goldens_regenerate_bit_identically(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(FLOW, "gen_flow_golden.py"), "--ref", REF, "--out", str(tmp_path)],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    made = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npz"))
    committed = sorted(f for f in os.listdir(FLOW) if f.endswith(".npz"))
    assert made == committed and len(made) == 7
    n = 0
    for f in made:
        a, b = np.load(os.path.join(tmp_path, f)), np.load(os.path.join(FLOW, f))
        assert sorted(a.files) == sorted(b.files), f
        for k in a.files:
            x, y = a[k], b[k]
            assert x.shape == y.shape and x.dtype == y.dtype, (f, k)
            assert np.array_equal(x, y), (f, k)
            n += 1
    assert n > 300
