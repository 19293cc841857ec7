"""AddressSanitizer + UndefinedBehaviorSanitizer on the CPU for the sampler update (GPU sanitizers are not available on this
pool): csrc/zs_mcmc_math.h is __host__ __device__; tests/host_math/zs_mcmc_host_math.hip, a stand-alone program with its own
main, is built for the host with the sanitizers and run directly -- nothing is preloaded, nothing is loaded into python.  It
holds every kind's arithmetic to long-double restatements over a grid of operands (a = 0, g = 0, hyper-parameters at their
extremes; the bound of tests/test_mcmc_kernel.py) and walks the element form's indexing (bisection, clamping, tail) over
exactly-sized heap arrays for that test's layouts."""
from host_math_runner import run_host_math


def test_sampler_arithmetic_and_indexing_on_the_host_under_asan_and_ubsan(tmp_path):
    run_host_math(tmp_path, "zs_mcmc_host_math.hip", "mcmc host math ok", 100000)
