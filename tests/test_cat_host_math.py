"""AddressSanitizer + UndefinedBehaviorSanitizer on the CPU for the categorical kernels (GPU sanitizers are not available on this
pool): csrc/zs_cat_math.h (with zs_group_math.h) is __host__ __device__; tests/host_math/zs_cat_host_math.hip, a stand-alone
program with its own main, is built for the host with the sanitizers and run directly -- nothing is preloaded, nothing is loaded
into python.  It holds the Gumbel transform at the smallest and the largest u01, the running (max, sum-exp) pair in the kernel's
own split orders for N up to 4099, and the densities at tau from 1e-3 to 1e3 to long-double restatements, and walks the
lane-group map of the kernels' loops over exactly-sized heap arrays for every N of tests/test_cat_kernel.py: each
(row, category) is owned exactly once."""
from host_math_runner import run_host_math


def test_cat_arithmetic_and_lane_group_maps_on_the_host_under_asan_and_ubsan(tmp_path):
    import zhusuan.distributions.categorical  # noqa: F401  (the feature under test)
    run_host_math(tmp_path, "zs_cat_host_math.hip", "cat host math ok", 50000)
