"""Every kernel of the satellite libraries (libzs_cat, libzs_mvn, libzs_klpq, libzs_hmc, libzs_flow) past its grid cap, through the
raw C ABI, against the float64 truths and the derived bounds of the libraries' own kernel test files.  See
tests/README_variants.md, "The satellite libraries".

Every satellite kernel is a grid-stride loop under a cap on the grid; the shapes of the other test files stay under every cap, so
the second trip of those loops never ran.  Each gate here is a pair: the smallest shape that takes a second trip ("over") and
its neighbour one row, datapoint, element or chain under it ("under").  Both sides run the owning file's check function
unchanged (truth, derived bound, guards around every output, the same call twice); on top of that

  * coverage: no output element keeps the fill of its buffer;
  * sibling: the leading rows / datapoints (cat, mvn, klpq) or the leading particles (mvn) of the "over" inputs, launched as a
    problem of their own that takes one trip, give the same bits.

``test_case_table_against_the_gates`` (not gpu) re-derives every shape from the block sizes and caps it reads from csrc/."""
import math
import os
import re

import numpy as np
import pytest
import torch

import test_cat_kernel as TC
import test_flow_kernel as TF
import test_hmc_kernel as TH
import test_klpq_kernel as TQ
import test_mvn_kernel as TM
from kernel_abi import DEV, F32, F64, SENTINEL, Arena, covered, load, load_main, ptr, same_bits, sfx, stream
from test_size_gated_variants import _stops_the_session_on_a_device_fault as stops_on_fault

gpu = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_MEMO = {}          # results of ONE pair at a time: the sibling test of a pair reads what its two sides left


def memo(pair_key, side_key, build):
    if _MEMO.get("pair") != pair_key:
        _MEMO.clear()
        _MEMO["pair"] = pair_key
    if side_key not in _MEMO:
        _MEMO[side_key] = build()
    return _MEMO[side_key]


# =====================================================================================================================
# the case table
# =====================================================================================================================
# libzs_cat: (id, N, R over, K, has an under neighbour); items = K R forward, R backward; 256 / G items per workgroup
CAT = [("G64-chunk", 129, 16385, 1, True), ("G64-strided", 257, 8193, 2, True), ("G64-bwd-particles", 129, 16385, 2, False),
       ("G16", 64, 65537, 1, True), ("G1", 3, 1048577, 1, True)]
CAT_WHICH = ["draw", "relaxed", "logmass_bwd", "relaxed_bwd"]
# libzs_mvn: (id, D, R over, K); 64 / G rows per workgroup
MVN_PAIRS = [("G64", 33, 4097, 5), ("G4", 3, 65537, 2), ("G1", 1, 262145, 2)]
# (id, D, R, K, kshare, gy, the smaller K' whose launches have kshare = 1)
MVN_SHARES = [("two-shares", 33, 1500, 5, 3, 2, (1, 2)), ("ragged-last-share", 5, 1, 2049, 2, 1025, (1, 5)),
              ("ragged-sibling", 5, 1, 2048, 1, 2048, (1, 5))]
# libzs_klpq: (id, K, B over, [(Tp, Tq, layout, scale)]); 256 / G datapoints per workgroup forward, 256 elements backward
KLPQ_PAIRS = [("G64", 65, 16385, [(2, 1, "sb0", 1.0), (3, 2, "sk0", 5.0)]),
              ("G4", 3, 262145, [(1, 1, "kb", 1.0), (3, 2, "mixed", 5.0)]),
              ("G1", 1, 1048577, [(1, 1, "bk", 1.0), (3, 2, "mixed", 0.0)])]
KLPQ_MEAN = [(K, 1024) for K in (1, 65)]
# libzs_hmc
HMC_DECIDE = [1024, 1025, 2051]          # 1024 is the neighbour under the second pass, 2051 takes a third
HMC_SELECT = [("element", 4194309, 0), ("element-under", 4194304, 1), ("vector", 4194308, 0), ("vector-under", 4194304, 0)]
HMC_MOVE = [("over", 16384 * 1024 + 5), ("under", 16384 * 1024)]
# libzs_flow: (id, B over, D, B under); the cap is 2048 workgroups of 256 items
FLOW_W4 = ("W4", 2049, 1024, 2048)          # items = B D / 4 (the 16-byte forms), B D / 2 (the pair kernels)
FLOW_W1 = ("W1", 682, 769, 681)             # items = B D (the element forms)
FLOW_TAIL = ("tail", 8193, 65, 8192)        # 4 rows per workgroup
FLOW_INV = ("inv-col", 524289, 2, 524288)   # one row per thread
FLOW_SCALE = [(3, 1024, 1), (3, 1025, 2), (3, 2049, 3)]          # (B, D, passes of the logdet sum)


# =====================================================================================================================
# the gates, restated from csrc/ (not gpu)
# =====================================================================================================================
def _src(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def _define(text, name):
    m = re.search(r"#define\s+%s\s+(\d+)\b" % name, text)
    assert m, "%s is no longer a plain #define" % name
    return int(m.group(1))


def _constexpr(text, name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)u?\s*;" % name, text)
    assert m, "%s is no longer a plain constexpr" % name
    return int(m.group(1))


def _cap(text, call):
    """the cap literal (`256u * 16u`) of the grid_for call whose first two arguments are `call`"""
    m = re.search(r"grid_for\(\s*%s\s*,\s*([0-9u* ]+)\)" % re.escape(call), text)
    assert m, "no grid_for(%s, <cap>) any more" % call
    v = 1
    for f in m.group(1).split("*"):
        v *= int(f.strip().rstrip("u"))
    return v


def gates():
    cat_h, cat = _src("zhusuan-pytorch_amd", "csrc", "zs_cat_math.h"), _src("zhusuan-pytorch_amd", "csrc", "zs_cat.hip")
    mvn_h, mvn = _src("zhusuan-pytorch_amd", "csrc", "zs_mvn_math.h"), _src("zhusuan-pytorch_amd", "csrc", "zs_mvn.hip")
    klpq_h, klpq = _src("zhusuan-pytorch_amd", "csrc", "zs_klpq_math.h"), _src("zhusuan-pytorch_amd", "csrc", "zs_klpq.hip")
    hmc_h, hmc = _src("include", "zs_hmc.h"), _src("zhusuan-pytorch_amd", "csrc", "zs_hmc.hip")
    flow_h, flow = _src("zhusuan-pytorch_amd", "csrc", "zs_flow_math.h"), _src("zhusuan-pytorch_amd", "csrc", "zs_flow.hip")
    g = dict(cat_threads=_define(cat_h, "ZS_CAT_THREADS"), cat_cap=_cap(cat, "items, THREADS / G"),
             mvn_threads=_define(mvn_h, "ZS_MVN_THREADS"), mvn_max_dim=_define(mvn_h, "ZS_MVN_MAX_DIM"),
             mvn_cap=_cap(mvn, "R, THREADS / G"),
             klpq_threads=_define(klpq_h, "ZS_KLPQ_THREADS"), klpq_mean_threads=_define(klpq_h, "ZS_KLPQ_MEAN_THREADS"),
             klpq_mean_max_b=_define(klpq_h, "ZS_KLPQ_MEAN_MAX_B"), klpq_wave=_define(klpq_h, "ZS_KLPQ_WAVE"),
             klpq_cap=_cap(klpq, "B, (int)threads / G"), klpq_bwd_cap=_cap(klpq, "K * B, ZS_KLPQ_THREADS"),
             hmc_tile=_define(hmc_h, "ZS_HMC_TILE"), hmc_decide=_constexpr(hmc, "DECIDE_THREADS"),
             hmc_move_cap=_cap(hmc, "tiles, 1"), hmc_select_cap=_cap(hmc, "groups, THREADS"),
             flow_block=_constexpr(flow, "kBlock"), flow_grid=_constexpr(flow, "kMaxGrid"),
             flow_col_tile=_define(flow_h, "ZS_FLOW_COL_TILE"), flow_row_lanes=_define(flow_h, "ZS_FLOW_ROW_LANES"))
    m = re.search(r"int64_t shares = \((\d+) \+ gx - 1\) / gx;", mvn)
    assert m, "the particle shares of k_mvn_forward are no longer cut at a literal"
    g["mvn_share_target"] = int(m.group(1))
    assert re.search(r"constexpr int THREADS = TILE / 4;", hmc) and re.search(r"const int64_t groups = \(n \+ 3\) / 4;", hmc)
    assert "flat_grid(((n) + 3) / 4)" in flow and "flat_grid(n / 2)" in flow and "flat_grid(B)" in flow
    assert "flat_grid((B + rows - 1) / rows * kBlock)" in flow and "const int rows = kBlock / 64;" in flow
    assert re.search(r"for \(int64_t c = tid; c < C; c \+= DECIDE_THREADS\)", hmc)
    assert re.search(r"for \(int64_t k = t; k < D; k \+= N\)", flow)
    return g


def pow2_lanes(n, most):
    g = 1
    while g < most and g < n:
        g <<= 1
    return g


def cat_group_lanes(N):
    return pow2_lanes((N + 3) >> 2, 64)


def grid_for(work, per_workgroup, cap):
    return max(1, min(-(-work // per_workgroup), cap))


def trips(work, per_workgroup, cap):
    """trips of the grid-stride loop in the workgroup that takes the most"""
    return -(-work // (grid_for(work, per_workgroup, cap) * per_workgroup))


def mvn_shares(g, D, R, K):
    """(gx, kshare, gy) of k_mvn_forward's launch"""
    G = pow2_lanes(D, g["mvn_max_dim"])
    gx = grid_for(R, g["mvn_threads"] // G, g["mvn_cap"])
    shares = min(-(-g["mvn_share_target"] // gx), K, 65535)
    kshare = -(-K // shares)
    return gx, kshare, -(-K // kshare)


def test_case_table_against_the_gates():
    g = gates()
    # libzs_cat
    for name, N, R, K, has_under in CAT:
        per = g["cat_threads"] // cat_group_lanes(N)
        fwd, bwd = trips(K * R, per, g["cat_cap"]), trips(R, per, g["cat_cap"])
        assert fwd == (3 if name == "G64-bwd-particles" else 2), (name, fwd)          # (that case is there for the backward)
        assert bwd == (1 if name == "G64-strided" else 2), (name, bwd)
        if has_under:
            assert trips(K * (R - 1), per, g["cat_cap"]) == 1 and trips(R - 1, per, g["cat_cap"]) == 1, name
            assert K * (R - 1) == g["cat_cap"] * per, name          # the neighbour fills the capped grid exactly
    assert [cat_group_lanes(c[1]) for c in CAT] == [64, 64, 64, 16, 1]
    assert (CAT[3][2] - 1) % (64 // 16) == 0          # G = 16: the over row is the first group of a wave, alone in the last trip
    # libzs_mvn
    for name, D, R, K in MVN_PAIRS:
        per = g["mvn_threads"] // pow2_lanes(D, g["mvn_max_dim"])
        assert trips(R, per, g["mvn_cap"]) == 2 and trips(R - 1, per, g["mvn_cap"]) == 1, name
        assert R - 1 == g["mvn_cap"] * per, name
    assert mvn_shares(g, 33, 4097, 5) == (4096, 5, 1)
    for name, D, R, K, kshare, gy, smaller in MVN_SHARES:
        assert trips(R, g["mvn_threads"] // pow2_lanes(D, g["mvn_max_dim"]), g["mvn_cap"]) == 1, name
        assert mvn_shares(g, D, R, K)[1:] == (kshare, gy), (name, mvn_shares(g, D, R, K))
        for k in smaller:
            assert mvn_shares(g, D, R, k)[1] == 1, (name, k)
    assert MVN_SHARES[0][3] % MVN_SHARES[0][4] == 2 and MVN_SHARES[1][3] % MVN_SHARES[1][4] == 1          # ragged last shares: 2 and 1
    # libzs_klpq
    for name, K, B, combos in KLPQ_PAIRS:
        per = g["klpq_threads"] // pow2_lanes(K, g["klpq_wave"])
        assert trips(B, per, g["klpq_cap"]) == 2 and trips(B - 1, per, g["klpq_cap"]) == 1, name
        assert B - 1 == g["klpq_cap"] * per, name
    assert trips(65 * 16385, g["klpq_threads"], g["klpq_bwd_cap"]) == 2          # the backward's element loop
    assert trips(3 * 262145, g["klpq_threads"], g["klpq_bwd_cap"]) == 1
    for K, B in KLPQ_MEAN:
        assert B == g["klpq_mean_max_b"]
        assert trips(B, g["klpq_mean_threads"] // pow2_lanes(K, g["klpq_wave"]), 1) == (64 if K == 65 else 1)          # one workgroup walks them all
    # libzs_hmc
    assert [-(-C // g["hmc_decide"]) for C in HMC_DECIDE] == [1, 2, 3]
    threads = g["hmc_tile"] // 4
    for name, n, shift in HMC_SELECT:
        t = trips((n + 3) // 4, threads, g["hmc_select_cap"])
        assert t == (1 if name.endswith("under") else 2), (name, t)
        assert (n % 4 == 0 and shift == 0) == name.startswith("vector"), name
    assert HMC_SELECT[1][1] == 4 * threads * g["hmc_select_cap"]
    assert [trips(-(-n // g["hmc_tile"]), 1, g["hmc_move_cap"]) for _, n in HMC_MOVE] == [2, 1]
    assert HMC_MOVE[1][1] == g["hmc_tile"] * g["hmc_move_cap"]
    # libzs_flow
    blk, cap = g["flow_block"], g["flow_grid"]
    name, B, D, Bu = FLOW_W4
    assert D % 4 == 0 and trips(B * D // 4, blk, cap) == 2 and trips(Bu * D // 4, blk, cap) == 1 and B - Bu == 1
    assert trips(B * D // 2, blk, cap) == 3 and trips(Bu * D // 2, blk, cap) == 2          # the pair kernels: a trip further on
    name, B, D, Bu = FLOW_W1
    assert D % 4 and trips(B * D, blk, cap) == 2 and trips(Bu * D, blk, cap) == 1 and B - Bu == 1
    name, B, D, Bu = FLOW_TAIL
    rows = blk // 64
    assert trips(B, rows, cap) == 2 and trips(Bu, rows, cap) == 1 and Bu == rows * cap
    name, B, D, Bu = FLOW_INV
    assert trips(B, blk, cap) == 2 and trips(Bu, blk, cap) == 1 and Bu == blk * cap
    per_pass = g["flow_col_tile"] * g["flow_row_lanes"]
    for B, D, passes in FLOW_SCALE:
        assert -(-D // per_pass) == passes, D
    assert [-(-D // g["flow_col_tile"]) for _, D, _ in FLOW_SCALE] == [16, 17, 33]


# =====================================================================================================================
# libzs_cat
# =====================================================================================================================
@pytest.fixture(scope="module")
def cat_lib():
    return load("cat")


@pytest.fixture(scope="module")
def main_lib():
    return load_main()


def cat_rows(d, R):
    """the leading R rows of every operand of a cat case"""
    return dict((k, (v[:R] if k == "logits" else v[:, :R]).contiguous()) for k, v in d.items())


def cat_params(ci, which):
    """(scale, tau, exp_space) of a case: the scales, temperatures and both spaces rotate over the cases"""
    wi = CAT_WHICH.index(which)
    return TC.SCALES[(ci + wi) % 3], TC.TAUS[(ci + wi) % 4], (ci + wi + 1) % 2


def cat_side(lib, ci, which, side):
    """The owning file's check of one kind on the over shape, or on the leading R - 1 rows of the same inputs."""
    name, N, R, K, has_under = CAT[ci]
    scale, tau, e = cat_params(ci, which)

    def build():
        d = memo(("cat", ci, which), "inputs", lambda: TC.case_inputs(N, R, K, scale, neg_inf=which in ("draw", "relaxed")))
        r = R if side == "over" else R - 1
        dd = d if side == "over" else cat_rows(d, r)
        kw = dict(dtypes=(F32, F64) if (ci == 0 and side == "over") else (F32,), shifts=(0, 1) if N == 64 else (0,), d=dd)
        if which == "draw":
            found = TC.check_draw_and_log_mass(lib, N, r, K, scale, **kw)
        elif which == "relaxed":
            found = TC.check_relaxed_draw_and_density(lib, N, r, K, scale, tau, e, **kw)
        elif which == "logmass_bwd":
            found = TC.check_log_mass_backward(lib, N, r, K, scale, **kw)
        else:
            found = TC.check_relaxed_backward(lib, N, r, K, scale, tau, e, **kw)
        for outs in found.values():
            covered(outs)
        return found[F32]
    return memo(("cat", ci, which), side, build)


CAT_SIDES = [(ci, w, s) for ci in range(len(CAT)) for w in CAT_WHICH for s in (("over", "under") if CAT[ci][4] else ("over",))]


@gpu
@pytest.mark.parametrize("ci,which,side", CAT_SIDES, ids=["%s-%s-%s" % (CAT[c][0], w, s) for c, w, s in CAT_SIDES])
@stops_on_fault
def test_cat_beyond_the_grid_cap(cat_lib, ci, which, side):
    cat_side(cat_lib, ci, which, side)


@gpu
@pytest.mark.parametrize("ci,which", [(c, w) for c, w, s in CAT_SIDES if s == "under"],
                         ids=["%s-%s" % (CAT[c][0], w) for c, w, s in CAT_SIDES if s == "under"])
@stops_on_fault
def test_cat_leading_rows_are_the_one_trip_launch(cat_lib, ci, which):
    name, N, R, K, _ = CAT[ci]
    over, under = cat_side(cat_lib, ci, which, "over"), cat_side(cat_lib, ci, which, "under")
    for a, b in zip(over, under):
        if a is None:
            continue
        if a.numel() in (K * R, K * R * N):          # per particle and row
            a = a.view(K, R, -1)[:, :R - 1].reshape(-1)
        else:                                        # summed over the particles: per row
            a = a.view(R, -1)[:R - 1].reshape(-1)
        assert same_bits(a, b), "the rows of the first trip differ from the one-trip launch (%s, %s)" % (name, which)


@gpu
@pytest.mark.parametrize("ci", range(len(CAT)), ids=[c[0] for c in CAT])
@stops_on_fault
def test_cat_drawn_noise_beyond_the_grid_cap(cat_lib, main_lib, ci):
    """C1 and C3 with u drawn in the kernel: the bits of the launch that is handed the main library's uniform stream."""
    name, N, R, K, has_under = CAT[ci]
    for r in (R, R - 1) if has_under else (R,):
        lg = TC.case_inputs(N, r, K, 1.0)["logits"]
        n = K * r * N
        seed, call = 11, 3
        noise = torch.empty(n, dtype=F32, device=DEV)
        main_lib.call("zs_philox_uniform_f32", noise.data_ptr(), n, seed, call, None, stream())
        ar = Arena(0)
        dl, du = ar.put(lg, F32), ar.put(noise.cpu(), F32)
        drawn = TC.c1(cat_lib, F32, ar, dl, None, K, r, N, seed=seed, call=call)
        given = TC.c1(cat_lib, F32, ar, dl, du, K, r, N)
        rdrawn = TC.c3(cat_lib, F32, ar, dl, None, 0.5, 1, K, r, N, seed=seed, call=call)
        rgiven = TC.c3(cat_lib, F32, ar, dl, du, 0.5, 1, K, r, N)
        ar.check_guards()
        for a, b in list(zip(drawn, given)) + list(zip(rdrawn, rgiven)):
            if isinstance(a, int):
                assert a == 0 and b == 0
            else:
                covered([a.cpu()])
                assert same_bits(a, b), "the in-kernel draw is not the injected Philox stream (%s, R=%d)" % (name, r)


@gpu
@pytest.mark.parametrize("n", [1048577, 1048576])
@stops_on_fault
def test_cat_exp_beyond_the_grid_cap(cat_lib, n):
    """zs_cat_exp (zs_cat.hip:563, 4096 workgroups of 256 elements) is the device exp that C3 applies to the y it stores: the
    first n elements of the G = 1 case's y give the first n of its exp(y), bit for bit, and every one of them is written."""
    name, N, R, K, _ = CAT[4]
    scale = 1.0
    d = TC.case_inputs(N, R, K, scale)
    ar = Arena(0)
    dl, du = ar.put(d["logits"], F32), ar.put(d["u"], F32)
    rc, y, ey, lp = TC.c3(cat_lib, F32, ar, dl, du, 0.5, 1, K, R, N)
    outs = [ar.out(n, F32) for _ in range(2)]
    for o in outs:
        assert cat_lib.raw("zs_cat_exp_f32", ptr(y), ptr(o), n, stream()) == 0
    ar.check_guards()
    covered([outs[0].cpu()])
    assert rc == 0 and same_bits(outs[0], outs[1]) and same_bits(outs[0], ey[:n])


# =====================================================================================================================
# libzs_mvn
# =====================================================================================================================
@pytest.fixture(scope="module")
def mvn_lib():
    return load("mvn")


def mvn_rows(d, R):
    return dict((k, (v[:R] if k in ("tril", "mean") else v[:, :R]).contiguous()) for k, v in d.items())


def mvn_side(lib, pi, side):
    name, D, R, K = MVN_PAIRS[pi]

    def build():
        d = memo(("mvn", pi), "inputs", lambda: TM.case_inputs(D, R, K))
        r = R if side == "over" else R - 1
        found = TM.check_forward_and_backward(lib, D, r, K, dtypes=(F32, F64) if (pi == 1 and side == "over") else (F32,),
                                              shifts=(0,), d=d if side == "over" else mvn_rows(d, r))
        for outs in found.values():
            covered(outs)
        return found[F32]
    return memo(("mvn", pi), side, build)


MVN_SIDES = [(pi, s) for pi in range(len(MVN_PAIRS)) for s in ("over", "under")]


@gpu
@pytest.mark.parametrize("pi,side", MVN_SIDES, ids=["%s-%s" % (MVN_PAIRS[p][0], s) for p, s in MVN_SIDES])
@stops_on_fault
def test_mvn_beyond_the_grid_cap(mvn_lib, pi, side):
    mvn_side(mvn_lib, pi, side)


@gpu
@pytest.mark.parametrize("pi", range(len(MVN_PAIRS)), ids=[p[0] for p in MVN_PAIRS])
@stops_on_fault
def test_mvn_leading_rows_are_the_one_trip_launch(mvn_lib, pi):
    name, D, R, K = MVN_PAIRS[pi]
    over, under = mvn_side(mvn_lib, pi, "over"), mvn_side(mvn_lib, pi, "under")
    for a, b in zip(over, under):
        a = a.view(K, R, -1)[:, :R - 1] if a.numel() in (K * R, K * R * D) else a.view(R, -1)[:R - 1]
        assert same_bits(a.reshape(-1), b), "the rows of the first trip differ from the one-trip launch (%s)" % name


def mvn_forward(lib, main_lib, d, D, R, K, drawn):
    """V1 (noise given, or drawn and compared with the launch that is given the main library's stream) and V2 on the leading K
    particles of `d`; returns (z, lp of V1, lp of V2) on the CPU."""
    ar = Arena(0)
    dm, dt, dx = ar.put(d["mean"], F32), ar.put(d["tril"], F32), ar.put(d["x"][:K], F32)
    seed, call = 11, 3
    if drawn:
        n = K * R * D
        noise = torch.empty(n, dtype=F32, device=DEV)
        main_lib.call("zs_philox_normal_f32", noise.data_ptr(), n, seed, call, None, stream())
        de = ar.put(noise.cpu(), F32)
        rc0, z0, lp0 = TM.v1(lib, F32, ar, dm, dt, None, K, R, D, seed=seed, call=call)
    else:
        de = ar.put(d["eps"][:K], F32)
    rc, z, lp = TM.v1(lib, F32, ar, dm, dt, de, K, R, D)
    rc2, lp2 = TM.v2(lib, F32, ar, dm, dt, dx, K, R, D)
    ar.check_guards()
    assert rc == 0 and rc2 == 0
    if drawn:
        assert rc0 == 0 and same_bits(z0, z) and same_bits(lp0, lp), "the in-kernel draw is not the injected Philox stream"
    outs = [z.cpu().view(K, R, D), lp.cpu().view(K, R), lp2.cpu().view(K, R)]
    covered(outs)
    return outs


@gpu
@pytest.mark.parametrize("si", range(len(MVN_SHARES)), ids=[s[0] for s in MVN_SHARES])
@stops_on_fault
def test_mvn_particle_shares(mvn_lib, main_lib, si):
    """k_mvn_forward with more than one particle per share (blockIdx.y, kshare > 1, a ragged last share): the truth, and "the
    cut changes no bit" -- z and lp of the leading K' particles are those of the same rows launched with K' particles, where
    every share holds one particle (the flat index k R + r does not depend on K)."""
    name, D, R, K, kshare, gy, smaller = MVN_SHARES[si]
    d = TM.case_inputs(D, R, K)
    found = TM.check_forward_and_backward(mvn_lib, D, R, K, dtypes=(F32,), shifts=(0,), d=d)
    covered(found[F32])
    for drawn in (False, True):
        full = mvn_forward(mvn_lib, main_lib, d, D, R, K, drawn)
        if not drawn:
            assert same_bits(full[0].reshape(-1), found[F32][0]) and same_bits(full[1].reshape(-1), found[F32][1])
        for k in smaller:
            part = mvn_forward(mvn_lib, main_lib, d, D, R, k, drawn)
            for a, b in zip(full, part):
                assert same_bits(a[:k], b), "the cut of the particles into shares changed a bit (%s, K' = %d)" % (name, k)


@gpu
@pytest.mark.parametrize("pi", range(len(MVN_PAIRS)), ids=[p[0] for p in MVN_PAIRS])
@stops_on_fault
def test_mvn_leading_particles_beyond_the_grid_cap(mvn_lib, main_lib, pi):
    """The sibling of a row pair with K > 1: the same rows with one particle, noise given and drawn."""
    name, D, R, K = MVN_PAIRS[pi]
    d = memo(("mvn", pi), "inputs", lambda: TM.case_inputs(D, R, K))
    for drawn in (False, True):
        full, part = mvn_forward(mvn_lib, main_lib, d, D, R, K, drawn), mvn_forward(mvn_lib, main_lib, d, D, R, 1, drawn)
        for a, b in zip(full, part):
            assert same_bits(a[:1], b), "the leading particle differs from the launch with one particle (%s)" % name


# =====================================================================================================================
# libzs_klpq
# =====================================================================================================================
@pytest.fixture(scope="module")
def klpq_lib():
    return load("klpq")


def klpq_check(lib, K, B, Tp, Tq, layout, scale, dtypes):
    d = TQ.case_inputs(K, B, Tp, Tq, layout, scale)
    for dtype in dtypes:
        runs = [TQ.run_case(lib, dtype, d, K, B, layout, shift, flipped) for shift, flipped in ((0, False), (1, True))]
        ref = runs[0]
        for name in ref:
            if tuple(runs[1][name].shape) == tuple(ref[name].shape):
                assert same_bits(ref[name], runs[1][name]), "%s differs between layouts / alignments (K=%d B=%d %s)" % (name, K, B, layout)
        covered(ref.values())
        tag = " [K=%d B=%d Tp=%d Tq=%d %s scale %g %s]" % (K, B, Tp, Tq, layout, scale, sfx(dtype))
        TQ.check_case(tag, dtype, d, K, B, ref, B <= TQ.MEAN_MAX_B)
    return d


KLPQ_SIDES = [(pi, ci, s) for pi in range(len(KLPQ_PAIRS)) for ci in range(2) for s in ("over", "under")]


def _klpq_id(pi, ci, s):
    Tp, Tq, layout, scale = KLPQ_PAIRS[pi][3][ci]
    return "%s-T%d%d-%s-%s" % (KLPQ_PAIRS[pi][0], Tp, Tq, layout, s)


@gpu
@pytest.mark.parametrize("pi,ci,side", KLPQ_SIDES, ids=[_klpq_id(*c) for c in KLPQ_SIDES])
@stops_on_fault
def test_klpq_beyond_the_grid_cap(klpq_lib, pi, ci, side):
    name, K, B, combos = KLPQ_PAIRS[pi]
    Tp, Tq, layout, scale = combos[ci]
    klpq_check(klpq_lib, K, B if side == "over" else B - 1, Tp, Tq, layout, scale,
               (F32, F64) if (pi == 0 and ci == 0 and side == "over") else (F32,))


@gpu
@pytest.mark.parametrize("pi,ci", [(p, c) for p, c, s in KLPQ_SIDES if s == "over"],
                         ids=[_klpq_id(p, c, "sibling") for p, c, s in KLPQ_SIDES if s == "over"])
@stops_on_fault
def test_klpq_leading_datapoints_are_the_one_trip_launch(klpq_lib, pi, ci):
    """The same term pointers and strides with B - 1 datapoints (one trip): the bits of the leading datapoints of the launch
    that takes two."""
    from zhusuan._klpq_hip import KlpqTerm
    name, K, B, combos = KLPQ_PAIRS[pi]
    Tp, Tq, layout, scale = combos[ci]
    d = TQ.case_inputs(K, B, Tp, Tq, layout, scale)
    ar = Arena(0)
    tabs, keep = {}, []
    for side in ("p", "q"):
        tab = (KlpqTerm * len(d[side]))()
        for i, t in enumerate(d[side]):
            store = TQ.storage(layout, side, i, len(d[side]), False)
            val = ar.put((t if store == "kb" else t.t()).contiguous(), F32)
            keep.append(val)
            TQ.term_row(tab[i], t, val, store, ar, F32, False)
        tabs[side] = tab
    got = []
    for b in (B, B - 1, B):
        o = [ar.out(b * K, F32), ar.out(b, F32), ar.out(b, F32), ar.out(b, F32)]
        assert klpq_lib.raw("zs_klpq_forward_f32", tabs["p"], Tp, tabs["q"], Tq, K, b, 0, *([ptr(t) for t in o] + [None, stream()])) == 0
        got.append(o)
    ar.check_guards()
    for full, part, again in zip(*got):
        covered([full.cpu(), part.cpu()])
        assert same_bits(full, again), "two identical launches differ"
        assert same_bits(full[:part.numel()], part), "the datapoints of the first trip differ from the one-trip launch (%s)" % name


KLPQ_MEAN_COMBOS = [(Tp, Tq, layout) for Tp, Tq in ((1, 1), (3, 2)) for layout in TQ.LAYOUTS]


@gpu
@pytest.mark.parametrize("K,B", KLPQ_MEAN, ids=["K%d-B%d" % c for c in KLPQ_MEAN])
@stops_on_fault
def test_klpq_batch_mean_at_its_limit(klpq_lib, K, B):
    """B = ZS_KLPQ_MEAN_MAX_B: the one workgroup with the batch mean walks every datapoint its LDS can hold; mean_cost against
    float64, bound / ess bit-equal to the launch of many workgroups (asserted by the owning file's run_case)."""
    for i, (Tp, Tq, layout) in enumerate(KLPQ_MEAN_COMBOS):
        klpq_check(klpq_lib, K, B, Tp, Tq, layout, TQ.SCALES[i % 3], (F32, F64))


# =====================================================================================================================
# libzs_hmc
# =====================================================================================================================
@pytest.fixture(scope="module")
def hmc_lib():
    return load("hmc")


@gpu
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("C", HMC_DECIDE)
@stops_on_fault
def test_hmc_decide_beyond_one_pass(hmc_lib, C, dtype):
    """More chains than k_hmc_decide has threads: a thread accumulates the acceptance of two or three chains before the tree."""
    k, l0, l1, u, t, out, acc, st = TH.check_decide(hmc_lib, dtype, C, 1)
    covered([out, st], fill=SENTINEL)
    assert bool(((acc == 0) | (acc == 1)).all())
    out2, acc2, st2 = TH.run_decide(hmc_lib, dtype, C, k, l0, l1, u, TH.state_block(), adapting=1)
    assert torch.equal(out, out2) and torch.equal(acc, acc2) and torch.equal(st, st2), "two identical calls differ"


@gpu
@pytest.mark.parametrize("C", HMC_DECIDE)
@stops_on_fault
def test_hmc_decide_drawn_uniforms_beyond_one_pass(hmc_lib, C):
    k, l0, l1, _ = TH.decide_inputs(C, 5)
    seed, call = 0xABCDEF12345, 17
    rs = torch.tensor([99, 1 << 20], dtype=torch.int64, device=DEV)
    for kw, stream_args in [(dict(seed=seed, call=call), (seed, call, None)), (dict(seed=1, call=3, rs=rs), (1, 3, rs))]:
        drawn = TH.run_decide(hmc_lib, F32, C, k, l0, l1, None, TH.state_block(), adapting=1, **kw)
        u = TH.philox("zs_philox_uniform_f32", C, *stream_args)
        given = TH.run_decide(hmc_lib, F32, C, k, l0, l1, u, TH.state_block(), adapting=1)
        assert all(torch.equal(a, b) for a, b in zip(drawn, given))


HMC_SELECT_RUNS = [s + (F32,) for s in HMC_SELECT] + [HMC_SELECT[0] + (F64,)]          # the float64 twin at one over-case


@gpu
@pytest.mark.parametrize("name,n,shift,dtype", HMC_SELECT_RUNS, ids=["%s-%s" % (s[0], "f32" if s[3] == F32 else "f64") for s in HMC_SELECT_RUNS])
@stops_on_fault
def test_hmc_select_beyond_the_grid_cap(hmc_lib, name, n, shift, dtype):
    q0, q, _, _ = TH.inputs(n, dtype, 13)
    for accept in (1, 0):
        acc = torch.tensor([accept], dtype=torch.int32, device=DEV)
        want = q if accept else q0
        res = []
        for rep in range(2):
            ar = Arena(shift)
            v0, v1, vo = ar.put(q0), ar.put(q), ar.put(torch.full_like(q, float("nan")))
            table = [dict(q0=v0, q=v1, q_out=vo, start=0, row=n)]
            assert TH.raw_select(hmc_lib, dtype, table, n, 1, acc) == 0
            ar.check_guards()
            res.append(vo.cpu())
            assert torch.equal(v0.cpu(), q0) and torch.equal(v1.cpu(), q), "an input was modified"
        assert torch.equal(res[0], want) and torch.equal(res[1], want)


def hmc_slots(ksum, terms, S, n):
    """Every slot of a one-chain, one-tensor workspace: slot t is the sum over tile t, to the owning file's bound for a sum of
    ZS_HMC_TILE terms; the slot after the last tile (pieces(n) counts one more than a row starting at 0 touches) is zero."""
    T = 1024
    tiles = -(-n // T)
    pad = tiles * T - n
    want = torch.cat([terms, torch.zeros(pad, dtype=F64)]).view(tiles, T).sum(1)
    bound = (T * 2.0 ** -24 + TH.rel(F32)) * torch.cat([S, torch.zeros(pad, dtype=F64)]).view(tiles, T).sum(1)
    got = ksum.double().view(-1)
    assert got.numel() == TH.hmc_host.pieces(n) == tiles + 1
    err = (got[:tiles] - want).abs()
    assert bool((err <= bound).all()), (float(err.max()), float((err / bound.clamp_min(1e-300)).max()))
    assert bool((got[tiles:] == 0).all())


@gpu
@pytest.mark.parametrize("kind", [TH.BEGIN, TH.END], ids=["begin", "end"])
@pytest.mark.parametrize("side,n", HMC_MOVE, ids=[m[0] for m in HMC_MOVE])
@stops_on_fault
def test_hmc_move_beyond_the_grid_cap(hmc_lib, side, n, kind):
    """One chain of 16384 x 1024 + 5 elements: 16385 tiles on a grid capped at 16384 workgroups."""
    data, (q2, p2, p02, ksum) = TH.check_kind(hmc_lib, F32, kind, 1, [n], 11 + kind, shifts=(0,))
    Q, P, G, Z = [t.double() for t in data]
    if kind == TH.BEGIN:
        hmc_slots(ksum, Z * Z, Z * Z, n)
    else:
        Sp = P.abs() + (0.5 * TH.EPS * G).abs()
        hmc_slots(ksum, (P + 0.5 * TH.EPS * G) ** 2, Sp * Sp, n)


@gpu
@pytest.mark.parametrize("side,n", HMC_MOVE, ids=[m[0] for m in HMC_MOVE])
@stops_on_fault
def test_hmc_drawn_momentum_beyond_the_grid_cap(hmc_lib, side, n):
    q, p, g, _ = TH.inputs(n, F32, 7)
    seed, call = 0x1234ABCD5678, 41
    drawn = TH.run_move(hmc_lib, F32, TH.BEGIN, 1, [n], 0, (q, p, g, torch.zeros(n)), inject=False, seed=seed, call=call)
    z = TH.philox("zs_philox_normal_f32", n, seed, call)
    tail = 4 * 4096
    assert torch.equal(drawn[2][-tail:], z[-tail:]), "the last 4096 Philox groups differ from the main library's stream"
    assert torch.equal(drawn[2], z)
    Z, G = z.double(), g.double()
    TH.within(drawn[1], Z + 0.5 * TH.EPS * G, Z.abs() + (0.5 * TH.EPS * G).abs(), F32)
    hmc_slots(drawn[3], Z * Z, Z * Z, n)


# =====================================================================================================================
# libzs_flow
# =====================================================================================================================
@pytest.fixture(scope="module")
def flow_lib():
    return load("flow")


def flow_shapes(case, twin=False):
    """[(id, B, D, dtype)] of a pair; the float64 twin runs at the over shape when asked for"""
    name, B, D, Bu = case
    out = [("%s-over" % name, B, D, F32), ("%s-under" % name, Bu, D, F32)]
    return out + ([("%s-over-f64" % name, B, D, F64)] if twin else [])


FLOW_FLAT = flow_shapes(FLOW_W4, twin=True) + flow_shapes(FLOW_W1)


@gpu
@pytest.mark.parametrize("name,B,D,dtype", FLOW_FLAT, ids=[c[0] for c in FLOW_FLAT])
@stops_on_fault
def test_flow_mask_beyond_the_grid_cap(flow_lib, name, B, D, dtype):
    TF.check_mask(flow_lib, dtype, B, D, "nonbinary", np.random.RandomState(11 + B))


@gpu
@pytest.mark.parametrize("sel", [0, 1])
@pytest.mark.parametrize("name,B,D,dtype", flow_shapes(FLOW_W4), ids=[c[0] for c in flow_shapes(FLOW_W4)])
@stops_on_fault
def test_flow_interleave_beyond_the_grid_cap(flow_lib, name, B, D, dtype, sel):
    TF.check_interleave(flow_lib, dtype, B, D, sel, np.random.RandomState(23 + B + sel))


FLOW_MADE = FLOW_FLAT + flow_shapes(FLOW_INV)


@gpu
@pytest.mark.parametrize("name,B,D,dtype", FLOW_MADE, ids=[c[0] for c in FLOW_MADE])
@stops_on_fault
def test_flow_made_beyond_the_grid_cap(flow_lib, name, B, D, dtype):
    TF.check_made(flow_lib, dtype, B, D, np.random.RandomState(41 + B))


FLOW_TAILS = FLOW_FLAT + flow_shapes(FLOW_TAIL)


@gpu
@pytest.mark.parametrize("base", [TF.NORMAL, TF.LOGISTIC], ids=["normal", "logistic"])
@pytest.mark.parametrize("name,B,D,dtype", FLOW_TAILS, ids=[c[0] for c in FLOW_TAILS])
@stops_on_fault
def test_flow_tail_beyond_the_grid_cap(flow_lib, name, B, D, dtype, base):
    TF.check_tail(flow_lib, dtype, B, D, base, np.random.RandomState(53 + B + base))


@gpu
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("B,D,passes", FLOW_SCALE, ids=["D%d" % c[1] for c in FLOW_SCALE])
@stops_on_fault
def test_flow_scale_logdet_beyond_one_pass(flow_lib, B, D, passes, dtype):
    """k_scale_fwd's logdet: a thread of workgroup 0 adds two or three elements of log_scale before the tree."""
    TF.check_scale(flow_lib, dtype, B, D, np.random.RandomState(37 + B))
