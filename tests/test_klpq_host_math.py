"""AddressSanitizer + UndefinedBehaviorSanitizer on the CPU for the inclusive-KL kernels (GPU sanitizers are not available on this
pool): csrc/zs_klpq_math.h (with zs_group_math.h) is __host__ __device__; tests/host_math/zs_klpq_host_math.hip, a stand-alone
program with its own main, is built for the host with the sanitizers and run directly -- nothing is preloaded, nothing is loaded
into python.  It runs a datapoint's reductions in the kernel's split order (lane partials, xor butterfly) against long double for
every K of tests/test_klpq_kernel.py at that test's scales and offsets, with one -inf particle and with all -inf; walks the lane
and row map for every (K, B) of the grid in both launch shapes (every (k, b) owned exactly once, a group never crosses its wave);
addresses the four term layouts over exactly-sized heap arrays, forward and backward (the whole per-thread body of the backward
kernel, broadcast sums against long double); and forms the batch mean in the first wave's order against long double."""
from host_math_runner import run_host_math


def test_klpq_arithmetic_lane_map_and_stride_addressing_on_the_host_under_asan_and_ubsan(tmp_path):
    import zhusuan.variational.inclusive_kl  # noqa: F401  (the feature under test)
    run_host_math(tmp_path, "zs_klpq_host_math.hip", "klpq host math ok", 20000)
