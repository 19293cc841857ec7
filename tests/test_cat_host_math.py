"""AddressSanitizer + UndefinedBehaviorSanitizer on the CPU for the categorical kernels (GPU sanitizers are not available on this
pool): csrc/zs_cat_math.h (with zs_flat_math.h) is __host__ __device__; tests/host_math/zs_cat_host_math.hip, a stand-alone
program with its own main, is built for the host with the sanitizers and run directly -- nothing is preloaded, nothing is loaded
into python.  It holds the Gumbel transform at the smallest and the largest u01, the running (max, sum-exp) pair in the kernel's
own split orders for N up to 4099, and the densities at tau from 1e-3 to 1e3 to long-double restatements, and walks the
lane-group map of the kernels' loops over exactly-sized heap arrays for every N of tests/test_cat_kernel.py: each
(row, category) is owned exactly once."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_cat_arithmetic_and_lane_group_maps_on_the_host_under_asan_and_ubsan(tmp_path):
    import zhusuan.distributions.categorical  # noqa: F401  (the feature under test)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "zs_cat_host_math")
    src = os.path.join(ROOT, "tests", "host_math", "zs_cat_host_math.hip")
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "cat host math ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert int(r.stdout.split("ok:")[1].split()[0]) > 50000
