"""AddressSanitizer + UndefinedBehaviorSanitizer on the CPU for Hamiltonian Monte Carlo (GPU sanitizers are not available on
this pool): csrc/zs_hmc_math.h is __host__ __device__; tests/host_math/zs_hmc_host_math.hip, a stand-alone program with its own
main, is built for the host with the sanitizers and run directly -- nothing is preloaded, nothing is loaded into python.  It
holds the leapfrog's arithmetic, dH, the acceptance probability, the decision and the dual-averaging recursion to long-double
restatements (g = 0, p = 0, eps at 1e-8 and 10, dH at +-800 and non-finite), and walks the chain-of-element map and the
partial-sum slot map of the kernel's tile loop over exactly-sized heap arrays for the layouts of tests/test_hmc_kernel.py."""
from host_math_runner import run_host_math


def test_hmc_arithmetic_and_index_maps_on_the_host_under_asan_and_ubsan(tmp_path):
    run_host_math(tmp_path, "zs_hmc_host_math.hip", "hmc host math ok", 100000)
