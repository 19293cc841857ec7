"""AddressSanitizer + UndefinedBehaviorSanitizer on the CPU for the planar / Householder flow kernels (GPU sanitizers are not
available on this pool): csrc/zs_nf_math.h (with zs_group_math.h) is __host__ __device__; tests/host_math/zs_nf_host_math.hip, a
stand-alone program with its own main, is built for the host with the sanitizers and run directly -- nothing is preloaded,
nothing is loaded into python.  It runs the parameter formulas (s in {-30, -3, 0, 3, 30}), one planar layer with its backward
pieces and the parameter chain (|a| up to 20) and one reflection with its backward in the kernels' own order against long double
for every D of tests/test_nf_kernel.py, and walks the lane-group and row-tile maps, the LDS places of z_l and the places of the
partial sums over exactly-sized heap arrays for every D, R in {1, 3, 65} and L in {1, 32}: every (row, i, l) is owned exactly
once, a group never crosses its wave, every partials element is written exactly once."""
from host_math_runner import run_host_math


def test_nf_arithmetic_and_lane_group_maps_on_the_host_under_asan_and_ubsan(tmp_path):
    import zhusuan.transform  # noqa: F401  (the feature under test)
    run_host_math(tmp_path, "zs_nf_host_math.hip", "nf host math ok", 20000)
