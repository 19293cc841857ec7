"""AddressSanitizer + UndefinedBehaviorSanitizer on the CPU for the multivariate-normal kernels (GPU sanitizers are not available
on this pool): csrc/zs_mvn_math.h (with zs_group_math.h) is __host__ __device__; tests/host_math/zs_mvn_host_math.hip, a
stand-alone program with its own main, is built for the host with the sanitizers and run directly -- nothing is preloaded,
nothing is loaded into python.  It runs the matvec, the two substitutions and the density in the kernels' own order against long
double for every D of tests/test_mvn_kernel.py, to that test's bounds, and walks the lane-group map, the walk of a group over a
row's matrix and the LDS tile places over exactly-sized heap arrays for every D and R in {1, 3, 65}: every (row, i) and every
(row, i >= j) is owned exactly once, nothing above the diagonal is read, and a group never crosses its wave."""
from host_math_runner import run_host_math


def test_mvn_arithmetic_and_lane_group_maps_on_the_host_under_asan_and_ubsan(tmp_path):
    import zhusuan.distributions.multivariate  # noqa: F401  (the feature under test)
    run_host_math(tmp_path, "zs_mvn_host_math.hip", "mvn host math ok", 20000)
