"""AddressSanitizer + UndefinedBehaviorSanitizer on the CPU for Hamiltonian Monte Carlo (GPU sanitizers are not available on
this pool): csrc/zs_hmc_math.h is __host__ __device__; tests/host_math/zs_hmc_host_math.hip, a stand-alone program with its own
main, is built for the host with the sanitizers and run directly -- nothing is preloaded, nothing is loaded into python.  It
holds the leapfrog's arithmetic, dH, the acceptance probability, the decision and the dual-averaging recursion to long-double
restatements (g = 0, p = 0, eps at 1e-8 and 10, dH at +-800 and non-finite), and walks the chain-of-element map and the
partial-sum slot map of the kernel's tile loop over exactly-sized heap arrays for the layouts of tests/test_hmc_kernel.py."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_hmc_arithmetic_and_index_maps_on_the_host_under_asan_and_ubsan(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "zs_hmc_host_math")
    src = os.path.join(ROOT, "tests", "host_math", "zs_hmc_host_math.hip")
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "hmc host math ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert int(r.stdout.split("ok:")[1].split()[0]) > 100000
