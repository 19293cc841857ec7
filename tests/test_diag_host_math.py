"""AddressSanitizer + UndefinedBehaviorSanitizer on the CPU for the chain-diagnostics kernels (GPU sanitizers are not available on
this pool): csrc/zs_diag_math.h (with zs_flat_math.h) is __host__ __device__; tests/host_math/zs_diag_host_math.hip, a stand-alone
program with its own main, is built for the host with the sanitizers and run directly -- nothing is preloaded, nothing is loaded
into python.  It runs the whole per-lane body of zs_diag_summary (the three passes over a strided series and the Geyer loop) over
exactly-sized heap arrays against long double for every (T, C, split, max_lag) of tests/test_diag_kernel.py in both stack orders
(the same bits), with every output and with each output alone; N = 2; a cap at an odd and at an even Lcap; more chains than a lane
keeps means of; a series with a NaN, one with an infinity and a constant one; the autocorrelation curve; and the stride check."""
from host_math_runner import run_host_math


def test_diag_arithmetic_and_stride_addressing_on_the_host_under_asan_and_ubsan(tmp_path):
    import zhusuan.diagnostics  # noqa: F401  (the feature under test)
    run_host_math(tmp_path, "zs_diag_host_math.hip", "diag host math ok", 3000)
