"""AddressSanitizer + UndefinedBehaviorSanitizer on the CPU for the planar / Householder flow kernels (GPU sanitizers are not
available on this pool): csrc/zs_nf_math.h (with zs_flat_math.h) is __host__ __device__; tests/host_math/zs_nf_host_math.hip, a
stand-alone program with its own main, is built for the host with the sanitizers and run directly -- nothing is preloaded,
nothing is loaded into python.  It runs the parameter formulas (s in {-30, -3, 0, 3, 30}), one planar layer with its backward
pieces and the parameter chain (|a| up to 20) and one reflection with its backward in the kernels' own order against long double
for every D of tests/test_nf_kernel.py, and walks the lane-group and row-tile maps, the LDS places of z_l and the places of the
partial sums over exactly-sized heap arrays for every D, R in {1, 3, 65} and L in {1, 32}: every (row, i, l) is owned exactly
once, a group never crosses its wave, every partials element is written exactly once."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_nf_arithmetic_and_lane_group_maps_on_the_host_under_asan_and_ubsan(tmp_path):
    import zhusuan.transform  # noqa: F401  (the feature under test)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "zs_nf_host_math")
    src = os.path.join(ROOT, "tests", "host_math", "zs_nf_host_math.hip")
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "nf host math ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert int(r.stdout.split("ok:")[1].split()[0]) > 20000
