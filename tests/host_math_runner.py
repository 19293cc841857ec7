"""What the tests/test_*_host_math.py files share: a program of tests/host_math/ -- stand-alone, with its own main -- is built for
the host with AddressSanitizer + UndefinedBehaviorSanitizer and run directly; nothing is preloaded, nothing is loaded into python."""
import os
import shutil
import subprocess

from conftest import ROOT


def run_host_math(tmp_path, source, marker, min_checks):
    """Build tests/host_math/<source>, run it, require `marker` and more than `min_checks` checks; returns the printed count."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / os.path.splitext(source)[0])
    src = os.path.join(ROOT, "tests", "host_math", source)
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-O1", "-g", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=all", src, "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and marker in r.stdout, (r.stdout + r.stderr)[-3000:]
    checks = int(r.stdout.split("ok:")[1].split()[0])
    assert checks > min_checks, (checks, min_checks)
    return checks
