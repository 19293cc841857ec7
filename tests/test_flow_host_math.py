"""AddressSanitizer + UndefinedBehaviorSanitizer on the CPU for the flow kernels (GPU sanitizers are not available on this
pool): csrc/zs_flow_math.h is __host__ __device__; tests/host_math/zs_flow_host_math.hip, a stand-alone program with its own
main, is built for the host with the sanitizers and run directly -- nothing is preloaded, nothing is loaded into python.  It
holds every formula to long-double restatements over a grid of operands (log_scale = +-80, zero and non-binary masks,
shift = 0; the bound of tests/test_flow_kernel.py) and walks the INTERLEAVE and strided-MADE index maps over exactly-sized heap
arrays for that test's shapes."""
from host_math_runner import run_host_math


def test_flow_arithmetic_and_index_maps_on_the_host_under_asan_and_ubsan(tmp_path):
    run_host_math(tmp_path, "zs_flow_host_math.hip", "flow host math ok", 20000)
