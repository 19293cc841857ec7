"""csrc/zs_svgd_math.h on the host: tests/host_math/zs_svgd_host_math.hip, a stand-alone program with its own main, is built for
the host with the sanitizers and run directly -- nothing is preloaded, nothing is loaded into python.  Exhaustively for
K = 1 .. 256 it walks the gram kernel's tile-pair <-> wave map over exactly-sized heap arrays, the padded-row mask, and the
bit-pattern selection of the median against a sorted array (ties, even and odd counts)."""
from host_math_runner import run_host_math


def test_svgd_index_maps_and_selection_on_the_host_under_asan_and_ubsan(tmp_path):
    run_host_math(tmp_path, "zs_svgd_host_math.hip", "svgd host math ok", 50000)
