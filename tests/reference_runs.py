"""TEST INFRASTRUCTURE shared by the test_*reference_suite.py and test_*golden_regeneration.py files: the run of the reference's
own test files against this package (in a subprocess, under tests/ref_plugin.py) and the bit-for-bit comparison of two fixture
directories.  Nothing of the reference is kept in this repository: its files are copied to a temporary directory at run time."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np

from conftest import ROOT, build_oracle_lib

REF = "/root/reference"


def run_reference_tests(tmp_path, files, targets, suite, env=None, timeout=900):
    """Copies ``files`` of the reference's ``test/`` tree to ``tmp_path/work/test`` and runs ``targets`` of them with pytest in a
    subprocess whose `zhusuan` is THIS package on the host back-end of ``suite`` ("", "flow" or "mcmc": tests/ref_plugin.py).
    Asserts that the run succeeded and returns the number of tests passed."""
    build_oracle_lib()
    work = tmp_path / "work"
    for rel in files:
        dst = work / "test" / rel
        dst.parent.mkdir(parents=True, exist_ok=True)
        shutil.copyfile(os.path.join(REF, "test", rel), dst)
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1", ZS_REF_SUITE=suite, **(env or {}))
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "tests"), os.path.join(ROOT, "zhusuan-pytorch_amd"), str(work)])
    cmd = [sys.executable, "-m", "pytest", "-p", "ref_plugin", "-p", "no:cacheprovider", "--rootdir", str(work), "-q"] + \
        (["-s"] if suite else []) + ["-W", "ignore"] + [str(work / "test" / t) for t in targets]
    r = subprocess.run(cmd, cwd=str(work), env=env, capture_output=True, text=True, timeout=timeout)
    tail = (r.stdout + r.stderr)[-3000:]
    print(tail)
    assert r.returncode == 0, tail
    passed = re.search(r"(\d+) passed", r.stdout.strip().splitlines()[-1])
    assert passed and "failed" not in r.stdout, tail
    return int(passed.group(1))


def same_fixtures(made_dir, committed_dir, equal_nan=False):
    """Asserts that the .npz files of the two directories have the same names, keys, shapes, dtypes and contents (a NaN equals
    a NaN only with ``equal_nan``, in float and complex arrays).  Returns the number of arrays compared."""
    made, committed = (sorted(f for f in os.listdir(d) if f.endswith(".npz")) for d in (made_dir, committed_dir))
    assert made == committed
    n = 0
    for f in made:
        a, b = np.load(os.path.join(made_dir, f)), np.load(os.path.join(committed_dir, f))
        assert sorted(a.files) == sorted(b.files), f
        for k in a.files:
            x, y = a[k], b[k]
            assert x.shape == y.shape and x.dtype == y.dtype, (f, k)
            assert np.array_equal(x, y, equal_nan=equal_nan and x.dtype.kind in "fc"), (f, k)
            n += 1
    return n
