"""The matrix-core libraries (libzs_mix, libzs_topic, libzs_svgd, libzs_matvar) past the one-trip shapes and the ladder ends of
their own kernel test files, through the raw C ABI, against the float64 truths and the derived bounds of those files.  See
tests/README_variants.md, "The matrix-core libraries".

At the shapes of test_mix_kernel.py, test_topic_kernel.py, test_svgd_kernel.py and test_matvar_kernel.py every strided loop whose
stride is a launch dimension takes one trip, and every host-side ladder that picks a template instantiation is entered at its
far ends only.  Each case here is the smallest shape that reaches one such loop or rung.  It runs the owning file's check
function unchanged (both element types, the aligned and the shifted Arena layout bit for bit, the guards, the same call twice,
the truth under the owning file's bound at the new shape); on top of that

  * coverage: no output element keeps the fill of its buffer;
  * sibling: what does not depend on the cut (lp, dx; lp, dB; a row's gradients at the same share length) is bit-identical
    across the cuts, what does is within the bound of the same truth at every cut.

``test_case_table_against_the_sources`` (not gpu) recomputes the trip count or the instantiation every line of ``TABLE`` claims
from the constants of csrc/; ``test_case_table_against_the_accessors`` (gpu) holds the same table to the libraries' accessors,
``test_svgd_case_reaches_its_instantiation`` to the kernel names torch.profiler reports."""
import os
import re

import pytest
import torch

import test_matvar_kernel as TV
import test_mix_kernel as TX
import test_svgd_kernel as TS
import test_topic_kernel as TT
from kernel_abi import ENOTSUP, F32, F64, Arena, covered, load, load_main, same_bits, sfx
from test_size_gated_variants import _kernels_of as kernels_of, _stops_the_session_on_a_device_fault as stops_on_fault

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOTH = (F32, F64)
_RESULTS = {}          # (library, case, cut) -> what the owning check function returned: a sibling test reads its sides here


def result(key, build):
    if key not in _RESULTS:
        _RESULTS[key] = build()
    return _RESULTS[key]


def report(case, worst):
    """the figures README_variants.md records"""
    print("TRIPS %s: %s" % (case, ", ".join("%s %.3f" % kv for kv in sorted(worst.items()))))


# =====================================================================================================================
# the case table
# =====================================================================================================================
MIX_WALK = (3, 17, 130)                     # (D, C, R): nine row tiles, the last of 2 rows
MIX_WALK_SHARES = (1, 2, 4)
MIX_CAP = (1, 65536, 33)                    # ZS_MIX_MAX_COMPONENTS: the library's own shares
TOPIC_WALK = (5, 1000, (2, 33), False)      # (K, V, (chains, docs), full X): 66 rows
TOPIC_WALK_SPLITS = (1, 3, None)            # None: the accessor's value
TOPIC_WIDE = (3, 70000, (1, 2), False)
TOPIC_ROWS = [(4, 17, (1, 300), False), (4, 17, (3, 100), False), (4, 17, (3, 100), True)]          # Dx = R, Dx < R, full X
SVGD_EDGE = [(48, BOTH), (49, BOTH), (64, BOTH), (113, BOTH), (128, BOTH), (129, (F32,)), (144, (F32,))]
SVGD_WALK = [(49, BOTH), (128, BOTH), (129, (F32,))]
# the update runs under a cap of its own, 1024 workgroups: 1027 slabs, so that three workgroups of each tier of the update stage a
# second slab over the first (and every workgroup of the Gram launch walks eight or nine)
SVGD_LONG_LAYOUT = [TS.SLAB * 1024 + 7, 2 * TS.SLAB - 3]
SVGD_LONG = [(17, BOTH), (49, BOTH), (129, (F32,))]
MATVAR = [(17, 15, 3, 19), (3, 2, 64, 19), (33, 3, 18, 7)]          # (n, p, R, K)

# One line per case: (case, kernel, the loop or ladder rung it is there for, the claim).  A claim is what
# test_case_table_against_the_sources recomputes: trips per workgroup (float32, float64 where they differ) or an instantiation.
TABLE = [
    ("mix (3, 17, 130) shares=1", "k_mix_grad_params", "rt += shares", dict(trips=[9], last_tile_rows=2)),
    ("mix (3, 17, 130) shares=2", "k_mix_grad_params", "rt += shares", dict(trips=[5, 4], last_tile_rows=2)),
    ("mix (3, 17, 130) shares=4", "k_mix_grad_params", "rt += shares", dict(trips=[3, 2, 2, 2], last_tile_rows=2)),
    ("mix (1, 65536, 33)", "k_mix_grad_params", "gridDim.x at the cap; rt += shares", dict(panels=(1024, 2048), shares=(1, 1), trips=[3])),
    ("topic (5, 1000, 2, 33) splits=1", "k_topic_grad_doc", "panel += splits", dict(trips=([16], [32]))),
    ("topic (5, 1000, 2, 33) splits=3", "k_topic_grad_doc", "panel += splits", dict(trips=([6, 5, 5], [11, 11, 10]))),
    ("topic (5, 1000, 2, 33) accessor", "k_topic_grad_doc", "panel += splits", dict(splits=(16, 32), trips=([1] * 16, [1] * 32))),
    ("topic (3, 70000, 1, 2)", "k_topic_grad_doc", "panel += splits", dict(panels=(1094, 2188), splits=(512, 512), trip_set=({2, 3}, {4, 5}))),
    ("topic (3, 70000, 1, 2)", "k_topic_grad_topic_finish", "p += 256; blockIdx.x > 0", dict(chunks=69, sum_trips=(5, 9))),
    ("topic (4, 17, 1, 300)", "k_topic_logprob_finish", "blockIdx.x > 0", dict(workgroups=2)),
    ("topic (4, 17, 3, 100)", "k_topic_logprob_finish", "blockIdx.x > 0, Dx < R", dict(workgroups=2)),
    ("svgd K=48", "k_svgd_gram, k_svgd_update", "the last K of PPW = 1", dict(nb=3, ppw=1, gram=1, update=(8, 8))),
    ("svgd K=49", "k_svgd_gram, k_svgd_update", "the first K of PPW = 5", dict(nb=4, ppw=2, gram=5, update=(8, 8), idle_slots=3)),
    ("svgd K=64", "k_svgd_gram, k_svgd_update", "nb = 4", dict(nb=4, ppw=2, gram=5, update=(8, 8), idle_slots=3)),
    ("svgd K=113", "k_svgd_gram, k_svgd_update", "the last rung of PPW = 5 and <8, 8>", dict(nb=8, ppw=5, gram=5, update=(8, 8))),
    ("svgd K=128", "k_svgd_gram, k_svgd_update", "the last K of PPW = 5 and <8, 8>", dict(nb=8, ppw=5, gram=5, update=(8, 8))),
    ("svgd K=129", "k_svgd_gram, k_svgd_update", "the first K of PPW = 17 and <16, 16>",
     dict(nb=9, ppw=6, gram=17, update=(16, 16), idle_slots=11, empty_waves=7)),
    ("svgd K=144", "k_svgd_gram, k_svgd_update", "nb = 9", dict(nb=9, ppw=6, gram=17, update=(16, 16), idle_slots=11, empty_waves=7)),
    ("svgd walk", "k_svgd_gram", "slab += gridDim.x", dict(slabs=131, workgroups=128, two_slabs=3)),
    ("svgd long", "k_svgd_update", "slab += gridDim.x", dict(slabs=1027, workgroups=1024, two_slabs=3, gram_trips={8, 9})),
    ("matvar (17, 15, 3, 19)", "k_matvar_sample_bwd, k_matvar_logprob_bwd", "k0 .. k1 with R > 1", dict(shares=10, per=2, last=1, row_per=2)),
    ("matvar (3, 2, 64, 19)", "k_matvar_sample_bwd, k_matvar_logprob_bwd", "the rows bound the shares", dict(shares=4, per=5, last=4, row_per=2)),
    ("matvar (33, 3, 18, 7)", "k_matvar_sample_bwd, k_matvar_logprob_bwd", "K bounds the shares just past the switch",
     dict(shares=7, per=1, last=1, row_per=1, target_shares=15)),
]


# =====================================================================================================================
# the arithmetic, restated from csrc/ (not gpu)
# =====================================================================================================================
def _src(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def _define(text, name):
    m = re.search(r"#define\s+%s\s+(\d+)\b" % name, text)
    assert m, "%s is no longer a plain #define" % name
    return int(m.group(1))


def constants():
    csrc = ("zhusuan-pytorch_amd", "csrc")
    tile, mix_h, topic_h = _src(*csrc, "zs_tile_math.h"), _src(*csrc, "zs_mix_math.h"), _src(*csrc, "zs_topic_math.h")
    matvar_h, svgd_h, svgd_api = _src(*csrc, "zs_matvar_math.h"), _src(*csrc, "zs_svgd_math.h"), _src("include", "zs_svgd.h")
    topic, svgd, mix = _src(*csrc, "zs_topic.hip"), _src(*csrc, "zs_svgd.hip"), _src(*csrc, "zs_mix.hip")
    m = re.search(r"PANEL = sizeof\(T\) == 4 \? (\d+) : (\d+)", tile)
    assert m, "MfmaPanel::PANEL is no longer a choice between two literals"
    c = dict(panel={4: int(m.group(1)), 8: int(m.group(2))},
             mix_target=_define(mix_h, "ZS_MIX_GRID_TARGET"), mix_max_c=_define(mix_h, "ZS_MIX_MAX_COMPONENTS"),
             topic_target=_define(topic_h, "ZS_TOPIC_GRID_TARGET"), topic_rows=_define(topic_h, "ZS_TOPIC_ROWS_PER_BLOCK"),
             matvar_target=_define(matvar_h, "ZS_MATVAR_GRID_TARGET"), matvar_max_shares=_define(matvar_h, "ZS_MATVAR_MAX_SHARES"),
             gram_waves=_define(svgd_h, "ZS_SVGD_GRAM_WAVES"), slab=_define(svgd_api, "ZS_SVGD_SLAB"),
             grid_cap=_define(svgd_api, "ZS_SVGD_GRID_CAP"),
             cap={4: _define(svgd_api, "ZS_SVGD_MAX_PARTICLES"), 8: _define(svgd_api, "ZS_SVGD_MAX_PARTICLES_F64")})
    m = re.search(r"constexpr int TOPIC_THREADS = (\d+);", topic)
    assert m, "TOPIC_THREADS is no longer a plain constexpr"
    c["topic_threads"] = int(m.group(1))
    # the loops the cases are there for, as text
    assert "for (int64_t rt = share; rt < tiles; rt += shares)" in mix
    assert "for (int64_t panel = blockIdx.y; panel < panels; panel += splits)" in topic
    assert "for (int64_t p = threadIdx.x; p < panels; p += TOPIC_THREADS)" in topic
    assert "const int64_t v = ((int64_t)blockIdx.x * 4 + i) * TOPIC_THREADS + threadIdx.x;" in topic
    assert "const int64_t r = (int64_t)blockIdx.x * TOPIC_THREADS + threadIdx.x;" in topic
    assert svgd.count("for (int64_t slab = blockIdx.x; slab < slabs; slab += gridDim.x)") == 2
    # the ladders of zs_svgd.hip: (threshold, instantiation), the last rung without a threshold
    g = re.search(r"if \(ppw <= (\d+)\) launch_gram<T, (\d+)>.*\n\s*else if \(ppw <= (\d+)\) launch_gram<T, (\d+)>.*\n\s*else if constexpr "
                  r"\(SvgdCap<T>::MAX_K > (\d+)\) launch_gram<T, (\d+)>", svgd)
    u = re.search(r"if \(nb <= (\d+)\) launch_update<T, (\d+), (\d+)>.*\n\s*else if \(nb <= (\d+)\) launch_update<T, (\d+), (\d+)>.*\n\s*else if "
                  r"constexpr \(SvgdCap<T>::MAX_K > (\d+)\) launch_update<T, (\d+), (\d+)>", svgd)
    assert g and u, "the ladders of svgd_gram / svgd_update have changed shape"
    g, u = [int(x) for x in g.groups()], [int(x) for x in u.groups()]
    c["gram_ladder"] = [(g[0], g[1]), (g[2], g[3]), (None, g[5])]
    c["update_ladder"] = [(u[0], (u[1], u[2])), (u[3], (u[4], u[5])), (None, (u[7], u[8]))]
    m = re.search(r"grid_for\(slabs, 1, (\d+)u\)", svgd)
    assert m, "the update's grid is no longer grid_for(slabs, 1, <cap>)"
    c["update_cap"] = int(m.group(1))
    c["wide_only_above"] = (g[4], u[6])          # the last rungs exist only where the element type's cap is above this
    return c


def ceil_div(a, b):
    return (a + b - 1) // b


def mix_row_shares(c, nb, R, C):
    return min(ceil_div(c["mix_target"], ceil_div(C, c["panel"][nb])), ceil_div(R, 16))


def topic_doc_splits(c, nb, R, V):
    return min(ceil_div(c["topic_target"], ceil_div(R, c["topic_rows"])), ceil_div(V, c["panel"][nb]))


def matvar_cut(c, K, R):
    """(shares, particles per share, particles of the last share, the share count before K and `no empty share` apply)"""
    target = min(ceil_div(c["matvar_target"], R), c["matvar_max_shares"])
    per = ceil_div(K, min(target, K))
    shares = ceil_div(K, per)
    return shares, per, K - (shares - 1) * per, ceil_div(c["matvar_target"], R)


def strided_trips(n, stride):
    """trips of `for (i = first; i < n; i += stride)` for first = 0 .. stride - 1"""
    return [len(range(first, n, stride)) for first in range(stride)]


def svgd_rungs(c, K):
    nb = ceil_div(K, 16)
    ppw = ceil_div(nb * (nb + 1) // 2, c["gram_waves"])
    gram = next(inst for most, inst in c["gram_ladder"] if most is None or ppw <= most)
    update = next(inst for most, inst in c["update_ladder"] if most is None or nb <= most)
    return nb, ppw, gram, update


def walk_layout():
    return TS.LAYOUTS["walk"]


def test_case_table_against_the_sources():
    c = constants()
    claims = {}
    for case, _, _, claim in TABLE:
        claims.setdefault(case, {}).update(claim)
    # mix
    D, C, R = MIX_WALK
    tiles = ceil_div(R, 16)
    assert R - 16 * (tiles - 1) == 2 and tiles == 9
    for shares in MIX_WALK_SHARES:
        cl = claims["mix (3, 17, 130) shares=%d" % shares]
        assert strided_trips(tiles, shares) == cl["trips"] and cl["last_tile_rows"] == 2
        assert shares <= tiles          # an accepted argument
    assert [mix_row_shares(c, nb, R, C) for nb in (4, 8)] == [tiles, tiles]          # what the owning file runs: one trip each
    D, C, R = MIX_CAP
    cl = claims["mix (1, 65536, 33)"]
    assert C == c["mix_max_c"]
    assert tuple(ceil_div(C, c["panel"][nb]) for nb in (4, 8)) == cl["panels"]
    assert tuple(mix_row_shares(c, nb, R, C) for nb in (4, 8)) == cl["shares"]
    assert strided_trips(ceil_div(R, 16), 1) == cl["trips"]
    # topic
    K, V, (chains, docs), _ = TOPIC_WALK
    R = chains * docs
    panels = [ceil_div(V, c["panel"][nb]) for nb in (4, 8)]
    for splits in (1, 3):
        assert tuple(strided_trips(p, splits) for p in panels) == claims["topic (5, 1000, 2, 33) splits=%d" % splits]["trips"]
    cl = claims["topic (5, 1000, 2, 33) accessor"]
    own = tuple(topic_doc_splits(c, nb, R, V) for nb in (4, 8))
    assert own == cl["splits"] == tuple(panels) and tuple(strided_trips(p, s) for p, s in zip(panels, own)) == cl["trips"]
    K, V, (chains, docs), _ = TOPIC_WIDE
    R = chains * docs
    cl = claims["topic (3, 70000, 1, 2)"]
    panels = tuple(ceil_div(V, c["panel"][nb]) for nb in (4, 8))
    own = tuple(topic_doc_splits(c, nb, R, V) for nb in (4, 8))
    assert panels == cl["panels"] and own == cl["splits"]
    assert tuple(set(strided_trips(p, s)) for p, s in zip(panels, own)) == cl["trip_set"]
    assert ceil_div(V, 4 * c["topic_threads"]) == cl["chunks"]
    assert tuple(max(strided_trips(p, c["topic_threads"])) for p in panels) == cl["sum_trips"]
    for K, V, (chains, docs), full in TOPIC_ROWS:
        assert ceil_div(chains * docs, c["topic_threads"]) == claims["topic (4, 17, %d, %d)" % (chains, docs)]["workgroups"] == 2
    assert [(ch * dc, ch * dc if full else dc) for _, _, (ch, dc), full in TOPIC_ROWS] == [(300, 300), (300, 100), (300, 300)]
    # svgd
    for K, dtypes in SVGD_EDGE:
        cl = claims["svgd K=%d" % K]
        nb, ppw, gram, update = svgd_rungs(c, K)
        assert (nb, ppw, gram, update) == (cl["nb"], cl["ppw"], cl["gram"], cl["update"]), K
        assert gram - ppw == cl.get("idle_slots", 0)          # accumulator slots of every wave that must stay idle
        if "empty_waves" in cl:
            assert update[1] - nb == cl["empty_waves"]          # waves of the update that own no strip
        assert update[0] >= nb and update[1] >= nb and gram >= ppw          # the tier holds K
        for dtype in dtypes:
            assert K <= c["cap"][4 if dtype == F32 else 8]
    assert svgd_rungs(c, 48)[2] != svgd_rungs(c, 49)[2] and svgd_rungs(c, 128)[2:] != svgd_rungs(c, 129)[2:]          # the rungs' edges
    assert svgd_rungs(c, 32)[3] != svgd_rungs(c, 33)[3]
    assert c["wide_only_above"] == (c["cap"][8], c["cap"][8]) and c["cap"][8] == 128          # K = 129 exists in float32 only
    assert all((F64 in dtypes) == (K <= c["cap"][8]) for K, dtypes in SVGD_EDGE + SVGD_WALK)
    cl = claims["svgd walk"]
    slabs = ceil_div(sum(walk_layout()), c["slab"])
    grid = min(slabs, c["grid_cap"])
    assert (slabs, grid) == (cl["slabs"], cl["workgroups"]) and strided_trips(slabs, grid).count(2) == cl["two_slabs"]
    assert max(strided_trips(slabs, grid)) == 2
    assert sorted({svgd_rungs(c, K)[2] for K, _ in SVGD_WALK}) == [5, 17] and {svgd_rungs(c, K)[3] for K, _ in SVGD_WALK} == {(8, 8), (16, 16)}
    cl = claims["svgd long"]
    slabs = ceil_div(sum(SVGD_LONG_LAYOUT), c["slab"])
    grid = min(slabs, c["update_cap"])
    assert (slabs, grid) == (cl["slabs"], cl["workgroups"]) and strided_trips(slabs, grid).count(2) == cl["two_slabs"]
    assert set(strided_trips(slabs, min(slabs, c["grid_cap"]))) == cl["gram_trips"]
    assert [svgd_rungs(c, K)[3] for K, _ in SVGD_LONG] == [(2, 4), (8, 8), (16, 16)]          # every tier of the update
    # matvar
    for n, p, R, K in MATVAR:
        cl = claims["matvar (%d, %d, %d, %d)" % (n, p, R, K)]
        shares, per, last, wanted = matvar_cut(c, K, R)
        assert (shares, per, last) == (cl["shares"], cl["per"], cl["last"]) and matvar_cut(c, K, 1)[1] == cl["row_per"]
        if "target_shares" in cl:
            assert wanted == cl["target_shares"] and K < wanted < c["matvar_max_shares"]
    assert ceil_div(c["matvar_target"], 64) < c["matvar_max_shares"]          # (3, 2, 64, 19): the rows bound the shares
    assert matvar_cut(c, 19, 3)[0] > 1 and matvar_cut(c, 19, 3)[1] > 1 and matvar_cut(c, 19, 3)[2] < matvar_cut(c, 19, 3)[1]          # walked, ragged


# =====================================================================================================================
# fixtures
# =====================================================================================================================
@pytest.fixture(scope="module")
def mix():
    return load("mix")


@pytest.fixture(scope="module")
def topic():
    return load("topic")


@pytest.fixture(scope="module")
def svgd():
    return load("svgd")


@pytest.fixture(scope="module")
def matvar():
    return load("matvar")


@pytest.fixture(scope="module")
def main_lib():
    return load_main()


@gpu
def test_case_table_against_the_accessors(mix, topic, svgd, matvar):
    c = constants()
    for nb in (4, 8):
        assert mix.raw("zs_mix_panels", nb, MIX_CAP[1]) == ceil_div(MIX_CAP[1], c["panel"][nb])
        for D, C, R in (MIX_WALK, MIX_CAP):
            assert mix.raw("zs_mix_row_shares", nb, R, C) == mix_row_shares(c, nb, R, C)
        for K, V, (chains, docs), _ in [TOPIC_WALK, TOPIC_WIDE] + TOPIC_ROWS:
            assert topic.raw("zs_topic_doc_splits", nb, chains * docs, V) == topic_doc_splits(c, nb, chains * docs, V)
            assert topic.raw("zs_topic_panels", nb, V) == ceil_div(V, c["panel"][nb])
    for n, p, R, K in MATVAR:
        assert matvar.raw("zs_matvar_shares", K, R) == matvar_cut(c, K, R)[0]
        assert matvar.raw("zs_matvar_shares", K, 1) == matvar_cut(c, K, 1)[0]
    assert svgd.raw("zs_svgd_gram_slots", sum(walk_layout())) == c["grid_cap"] == TS.CAP
    assert svgd.raw("zs_svgd_gram_slots", sum(TS.LAYOUTS["edge"])) == 2
    assert svgd.raw("zs_svgd_gram_slots", sum(SVGD_LONG_LAYOUT)) == c["grid_cap"]
    assert [svgd.raw("zs_svgd_max_particles_of", nb) for nb in (4, 8)] == [c["cap"][4], c["cap"][8]]
    assert mix.raw("zs_mix_max_components") == c["mix_max_c"]


# =====================================================================================================================
# libzs_mix
# =====================================================================================================================
def mix_case(lib, shape, shares):
    return result(("mix", shape, shares), lambda: TX.check_case(lib, *shape, shares=shares))


@gpu
@pytest.mark.parametrize("shares", MIX_WALK_SHARES)
@stops_on_fault
def test_mix_row_tiles_walked(mix, shares):
    outs, worst = mix_case(mix, MIX_WALK, shares)
    for dtype in BOTH:
        covered(outs[dtype])
    report("mix %s shares=%d" % (MIX_WALK, shares), worst)


@gpu
@stops_on_fault
def test_mix_shares_are_siblings(mix):
    """lp and dx do not depend on the cut: the same bits at every `shares`; the parameter gradients at one share and at a share
    per row tile are both within the bound of the same truth (check_case holds them to it)."""
    tiles = (MIX_WALK[2] + 15) // 16
    sides = {s: mix_case(mix, MIX_WALK, s)[0] for s in MIX_WALK_SHARES + (tiles,)}
    assert mix.raw("zs_mix_row_shares", 4, MIX_WALK[2], MIX_WALK[1]) == tiles
    for dtype in BOTH:
        covered(sides[tiles][dtype])
        for s in MIX_WALK_SHARES[1:]:
            for i, name in enumerate(TX.NAMES[:2]):
                assert same_bits(sides[1][dtype][i], sides[s][dtype][i]), "%s%s changes with the shares (%d)" % (name, sfx(dtype), s)


@gpu
@stops_on_fault
def test_mix_at_the_component_cap(mix):
    D, C, R = MIX_CAP
    assert [mix.raw("zs_mix_row_shares", nb, R, C) for nb in (4, 8)] == [1, 1]
    outs, worst = mix_case(mix, MIX_CAP, None)
    for dtype in BOTH:
        covered(outs[dtype])
    report("mix %s" % (MIX_CAP,), worst)


@gpu
@stops_on_fault
def test_mix_above_the_component_cap_writes_nothing(mix):
    D, C, R = MIX_CAP[0], MIX_CAP[1] + 1, MIX_CAP[2]
    ins = TX.case_inputs(D, C, R)
    for dtype in BOTH:
        ar = Arena(0)
        ops = [ar.put(a, dtype) for a in ins]
        rcs, _ = TX.run(mix, dtype, ar, ops, R, C, D, shares=1)
        assert rcs == [ENOTSUP] * 4
        ar.check_guards()
        assert ar.untouched(), "a rejected call wrote something"


# =====================================================================================================================
# libzs_topic
# =====================================================================================================================
def topic_case(lib, case, splits):
    return result(("topic", case, splits), lambda: TT.check_case(lib, *case, splits=splits))


def topic_name(case):
    return "topic (%d, %d, %d, %d)%s" % (case[0], case[1], case[2][0], case[2][1], " full X" if case[3] else "")


@gpu
@pytest.mark.parametrize("splits", TOPIC_WALK_SPLITS, ids=lambda s: "accessor" if s is None else "splits%d" % s)
@stops_on_fault
def test_topic_panels_walked(topic, splits):
    outs, worst = topic_case(topic, TOPIC_WALK, splits)
    for dtype in BOTH:
        covered(outs[dtype])
    report("%s splits=%s" % (topic_name(TOPIC_WALK), "accessor" if splits is None else splits), worst)


@gpu
@stops_on_fault
def test_topic_splits_are_siblings(topic):
    """lp and dB do not depend on the cut of grad_doc: the same bits at every `splits`; dH is within the bound at each."""
    sides = {s: topic_case(topic, TOPIC_WALK, s)[0] for s in TOPIC_WALK_SPLITS}
    for dtype in BOTH:
        for s in TOPIC_WALK_SPLITS[1:]:
            for i, name in ((0, "lp"), (2, "dB")):
                assert same_bits(sides[1][dtype][i], sides[s][dtype][i]), "%s%s changes with the splits (%s)" % (name, sfx(dtype), s)


@gpu
@pytest.mark.parametrize("case", [TOPIC_WIDE] + TOPIC_ROWS, ids=lambda c: "K%d-V%d-%dx%d%s" % (c[0], c[1], c[2][0], c[2][1], "-full" if c[3] else ""))
@stops_on_fault
def test_topic_beyond_one_trip(topic, case):
    outs, worst = topic_case(topic, case, None)
    for dtype in BOTH:
        covered(outs[dtype])
    report(topic_name(case), worst)


# =====================================================================================================================
# libzs_svgd
# =====================================================================================================================
SVGD_CASES = [(K, "edge", mu, dtype) for K, dtypes in SVGD_EDGE for mu in (0, 100) for dtype in dtypes] + \
             [(K, "walk", 100 * (i % 2), dtype) for i, (K, dtypes) in enumerate(SVGD_WALK) for dtype in dtypes] + \
             [(K, "long", 100 * (i % 2), dtype) for i, (K, dtypes) in enumerate(SVGD_LONG) for dtype in dtypes]


@gpu
@pytest.mark.parametrize("K,layout,mu,dtype", SVGD_CASES, ids=lambda v: sfx(v)[1:] if isinstance(v, torch.dtype) else str(v))
@stops_on_fault
def test_svgd_ladder_rungs_and_walk(svgd, K, layout, mu, dtype):
    thetas, grads = TS.inputs(K, SVGD_LONG_LAYOUT if layout == "long" else TS.LAYOUTS[layout], mu)
    worst = {}
    TS.check_step(svgd, dtype, K, thetas, grads, None, " [K=%d %s mu=%d %s]" % (K, layout, mu, sfx(dtype)), worst)
    report("svgd K=%d %s mu=%d %s" % (K, layout, mu, sfx(dtype)), worst)


@gpu
@pytest.mark.parametrize("K,dtype", [(K, dtype) for K, dtypes in SVGD_EDGE for dtype in dtypes],
                         ids=lambda v: sfx(v)[1:] if isinstance(v, torch.dtype) else str(v))
@stops_on_fault
def test_svgd_case_reaches_its_instantiation(svgd, K, dtype):
    nb, ppw, gram, update = svgd_rungs(constants(), K)
    thetas, grads = TS.inputs(K, TS.LAYOUTS["edge"], 0)
    ar = Arena(0)
    q, g = [ar.put(a, dtype) for a in thetas], [ar.put(a, dtype) for a in grads]
    rcs = []
    ours, names = kernels_of(lambda: rcs.append(TS.step(svgd, dtype, ar, K, q, g)[0]))
    assert rcs == [[0, 0, 0]]
    elem = "float" if dtype == F32 else "double"
    ran = [re.search(r"k_svgd_\w+(<[^>]*>)?", n).group(0) for n in ours if "k_svgd_" in n]
    print("K=%d %s -> %s" % (K, sfx(dtype), ran))
    assert ran == ["k_svgd_gram<%s, %d>" % (elem, gram), "k_svgd_finish", "k_svgd_update<%s, %d, %d>" % ((elem,) + update)], (ran, names)


# =====================================================================================================================
# libzs_matvar
# =====================================================================================================================
GRADS = ("gm1", "gu1", "gv1", "gm2", "gu2", "gv2")


def matvar_case(lib, main_lib, case):
    return result(("matvar", case), lambda: TV.check_case(lib, main_lib, *case, BOTH))


@gpu
@pytest.mark.parametrize("n,p,R,K", MATVAR)
@stops_on_fault
def test_matvar_walked_shares_over_rows(matvar, main_lib, n, p, R, K):
    outs, worst = matvar_case(matvar, main_lib, (n, p, R, K))
    for dtype in BOTH:
        covered(list(outs[dtype].values()))
    report("matvar (%d, %d, %d, %d)" % (n, p, R, K), worst)


@gpu
@pytest.mark.parametrize("n,p,R,K", MATVAR)
@stops_on_fault
def test_matvar_rows_are_their_one_row_problems(matvar, main_lib, n, p, R, K):
    """The gradients of row r against the one-row problem made of row r alone: the same bits where the two launches cut the
    particles into shares of the same length, else within the bound of the same truth."""
    outs, _ = matvar_case(matvar, main_lib, (n, p, R, K))
    d, t = TV.case_truth(n, p, R, K)
    shares, shares1 = matvar.raw("zs_matvar_shares", K, R), matvar.raw("zs_matvar_shares", K, 1)
    same_cut = (K + shares - 1) // shares == (K + shares1 - 1) // shares1
    worst = {}
    for dtype in BOTH:
        tol = TV.bounds(dtype, d, t, K)
        for r in range(R):
            one = {k: (v[r:r + 1] if k in ("U", "V", "mean") else v[:, r:r + 1]).contiguous() for k, v in d.items()}
            ar = Arena(0)
            o = {k: ar.put(v, dtype) for k, v in one.items()}
            a, b = TV.m1(matvar, dtype, ar, o, K, 1, n, p, o["eps"]), TV.m2(matvar, dtype, ar, o, K, 1, n, p, o["x"])
            ar.check_guards()
            assert a[0] == [0, 0] and b[0] == [0, 0]
            got = dict(zip(GRADS, [x.cpu() for x in a[3:] + b[3:]]))
            covered(list(got.values()))
            for k in GRADS:
                whole = outs[dtype][k].view(t[k].shape)[r]
                if same_cut:
                    assert same_bits(got[k].view(whole.shape), whole.contiguous()), "%s%s of row %d is not that of the row alone" % (k, sfx(dtype), r)
                else:
                    worst[k + sfx(dtype)] = max(worst.get(k + sfx(dtype), 0.0),
                                                TV.assert_close("%s [row %d alone, n=%d p=%d K=%d %s]" % (k, r, n, p, K, sfx(dtype)), got[k],
                                                                t[k][r], tol[k][r]))
    report("matvar (%d, %d, %d, %d) rows alone, %s" % (n, p, R, K, "bit-identical" if same_cut else "another share length"), worst)
