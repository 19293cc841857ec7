"""AddressSanitizer + UndefinedBehaviorSanitizer on the CPU for the inclusive-KL kernels (GPU sanitizers are not available on this
pool): csrc/zs_klpq_math.h (with zs_flat_math.h) is __host__ __device__; tests/host_math/zs_klpq_host_math.hip, a stand-alone
program with its own main, is built for the host with the sanitizers and run directly -- nothing is preloaded, nothing is loaded
into python.  It runs a datapoint's reductions in the kernel's split order (lane partials, xor butterfly) against long double for
every K of tests/test_klpq_kernel.py at that test's scales and offsets, with one -inf particle and with all -inf; walks the lane
and row map for every (K, B) of the grid in both launch shapes (every (k, b) owned exactly once, a group never crosses its wave);
addresses the four term layouts over exactly-sized heap arrays, forward and backward (the whole per-thread body of the backward
kernel, broadcast sums against long double); and forms the batch mean in the first wave's order against long double."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_klpq_arithmetic_lane_map_and_stride_addressing_on_the_host_under_asan_and_ubsan(tmp_path):
    import zhusuan.variational.inclusive_kl  # noqa: F401  (the feature under test)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "zs_klpq_host_math")
    src = os.path.join(ROOT, "tests", "host_math", "zs_klpq_host_math.hip")
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "klpq host math ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert int(r.stdout.split("ok:")[1].split()[0]) > 20000
