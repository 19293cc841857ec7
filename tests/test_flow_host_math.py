"""AddressSanitizer + UndefinedBehaviorSanitizer on the CPU for the flow kernels (GPU sanitizers are not available on this
pool): csrc/zs_flow_math.h is __host__ __device__; tests/host_math/zs_flow_host_math.hip, a stand-alone program with its own
main, is built for the host with the sanitizers and run directly -- nothing is preloaded, nothing is loaded into python.  It
holds every formula to long-double restatements over a grid of operands (log_scale = +-80, zero and non-binary masks,
shift = 0; the bound of tests/test_flow_kernel.py) and walks the INTERLEAVE and strided-MADE index maps over exactly-sized heap
arrays for that test's shapes."""
import os
import shutil
import subprocess

from conftest import ROOT


def test_flow_arithmetic_and_index_maps_on_the_host_under_asan_and_ubsan(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "zs_flow_host_math")
    src = os.path.join(ROOT, "tests", "host_math", "zs_flow_host_math.hip")
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "flow host math ok" in r.stdout, (r.stdout + r.stderr)[-3000:]
    assert int(r.stdout.split("ok:")[1].split()[0]) > 20000
