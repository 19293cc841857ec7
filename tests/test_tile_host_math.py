"""csrc/zs_tile_math.h on the host: tests/host_math/zs_tile_host_math.hip, a stand-alone program with its own main, is built for
the host with the sanitizers and run directly -- nothing is preloaded, nothing is loaded into python.  For float and double it
walks the accumulator row map of the matrix instruction over an exactly-sized heap tile (every element once; rows 2 t and 2 t + 1
neighbours, as the mix kernels' gradients need them), the panel arithmetic and the 16-wide round-up with the four libraries' sizes
built on them, and computes the LDS bank figures that the headers' comments quote for the paddings of the topic / mix panel, of
matvar's tile and of svgd's two tiles."""
from host_math_runner import run_host_math


def test_tile_map_panels_and_bank_figures_on_the_host_under_asan_and_ubsan(tmp_path):
    run_host_math(tmp_path, "zs_tile_host_math.hip", "tile host math ok", 6500)
