"""The Philox streams of every drawing entry point against a truth that is independent of both libraries
(tests/README_rng.md).

Truth: a vectorised numpy Philox4x32-10 in uint64 arithmetic (`philox_words`, pinned by the Random123 known answers),
and from its words, in float64, the uniform u = ((w >> 9) + 0.5) 2^-23 and the Box-Muller quadruple as the comment
above philox_normal4 (csrc/zs_common.h) defines it: radius from u01(x) / u01(z), angle from the upper 23 bits of y / w.
Every check runs on the C oracle (not gpu) and on libzs_hip.so (gpu); the SG-MCMC and HMC libraries exist on the GPU only.

Bounds.  Uniform and Bernoulli draws: bit for bit (the header's claim).  Normal draws: the unit-scale bound of
test_cabi.py::test_hip_rng carried to the radius, |got - truth| <= 3e-5 max(1, r), r = sqrt(-2 ln u) in float64 (an
error of v_cos / v_sin multiplies by r, nothing else in the formula does); a Logistic draw log u - log(1 - u) is held to
the same expression with the r of its own u.  _f64: the bounds test_cabi.py::test_hip_f64_entry_points uses for its
draws, 3e-5 for zs_philox_normal_f64 and 3e-4 sigma for zs_normal_sample_logprob_f64."""
import ctypes
import functools

import numpy as np
import pytest
import torch
from scipy import special, stats

from conftest import host_kernel_library
from test_cabi import PAIR_SHAPES
from test_locscale import Raw2
from zhusuan import _hip
import zhusuan as zs

U64 = np.uint64
M32 = U64(0xFFFFFFFF)
TWO_PI = 6.283185307179586476925
ATOL = 3e-5            # test_cabi.py::test_hip_rng, at unit scale
ATOL_F64_STREAM = 3e-5   # test_cabi.py::test_hip_f64_entry_points: hip64.philox
ATOL_F64_SAMPLE = 3e-4   # test_cabi.py::test_hip_f64_entry_points: hip64.normal_sample (times sigma = 1)


# ------------------------------------------------------------------------------------------------ the truth
def philox_words(group, call, seed):
    """Philox4x32-10 (Random123; Salmon et al. 2011): counter (lo group, hi group, lo call, hi call), key (lo seed, hi seed).
    `group`: array of uint64; returns uint64 [len(group), 4] holding the four 32-bit words."""
    g = np.asarray(group, dtype=U64)
    call, seed = int(call) & (2 ** 64 - 1), int(seed) & (2 ** 64 - 1)
    c0, c1 = g & M32, g >> U64(32)
    c2, c3 = np.full_like(c0, call & 0xFFFFFFFF), np.full_like(c0, call >> 32)
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = U64(0xD2511F53) * c0, U64(0xCD9E8D57) * c2        # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> U64(32)) ^ c1 ^ U64(k0), p1 & M32, (p0 >> U64(32)) ^ c3 ^ U64(k1), p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1)


def _u_of(w):
    return ((w >> U64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


@functools.lru_cache(maxsize=3)          # (an entry of 2^22 draws holds 128 MiB)
def _truth(n, call, seed):
    """(u, normal, r) of flat elements [0, n) of stream (seed, call): float64, read-only.  Element i is word i & 3 of
    group i >> 2; r is the Box-Muller radius of the normal at i."""
    w = philox_words(np.arange((n + 3) // 4, dtype=U64), call, seed)
    u = _u_of(w)
    ra, rb = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    a1 = TWO_PI * ((w[:, 1] >> U64(9)).astype(np.float64) * 2.0 ** -23)
    a3 = TWO_PI * ((w[:, 3] >> U64(9)).astype(np.float64) * 2.0 ** -23)
    z = np.stack([ra * np.cos(a1), ra * np.sin(a1), rb * np.cos(a3), rb * np.sin(a3)], axis=1)
    r = np.stack([ra, ra, rb, rb], axis=1)
    ur = np.stack([u[:, 0], u[:, 0], u[:, 2], u[:, 2]], axis=1)          # the uniform behind the radius of element i
    out = tuple(a.reshape(-1)[:n] for a in (u, z, r, ur))
    for a in out:
        a.setflags(write=False)
    return out


def truth_u(n, call, seed):
    return _truth(n, call, seed)[0]


def truth_normal(n, call, seed):
    """(normal, r, u behind r)"""
    return _truth(n, call, seed)[1:]


def test_truth_philox_known_answers():
    # the Random123 known-answer vectors quoted in test_cabi.py::test_philox_known_answers: (group, call, seed)
    kat = [((0, 0, 0), [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ((2 ** 64 - 1,) * 3, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ((0x85a308d3243f6a88, 0x0370734413198a2e, 0x299f31d0a4093822), [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for (g, c, s), want in kat:
        assert philox_words(np.array([g], dtype=U64), c, s)[0].tolist() == want
    # ... and agrees with the oracle's own generator on an id with every word set, over many groups
    orc = ctypes.CDLL(host_kernel_library().path)
    f = orc.zs_oracle_philox4x32_10
    f.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint32)]
    f.restype = None
    out = (ctypes.c_uint32 * 4)()
    groups = [0, 1, 5, 2 ** 32 - 1, 2 ** 32, 2 ** 34 + 3, 2 ** 63 + 1]       # group >= 2^32: covered here and only here
    w = philox_words(np.array(groups, dtype=U64), 2 ** 63 + 5, 2 ** 64 - 1)
    for g, row in zip(groups, w):
        f(g, 2 ** 63 + 5, 2 ** 64 - 1, out)
        assert list(out) == row.tolist()
    u = truth_u(1 << 12, 9, 1234)
    assert u.min() >= 2.0 ** -24 and u.max() <= 1 - 2.0 ** -24


# ------------------------------------------------------------------------------------------------ ids
TORCH_DEFAULT_SEED = 67280421310721          # upper word 0x3D30


class Ident(object):
    """One way of handing (seed, call) to an entry point, and the (seed, call) the stream must then be."""

    def __init__(self, label, seed, call, state=None, masked=False):
        self.label, self.masked = label, masked
        if state is None:
            self.by_value, self.state = (seed, call), None
            self.seed, self.call = seed, call
        else:                                  # {seed, base} in memory + offset by value; the by-value seed is ignored
            self.by_value, self.state = (7, call), state
            self.seed, self.call = (state[0] & (2 ** 63 - 1) if masked else state[0]), (state[1] + call) & (2 ** 64 - 1)

    def kw(self, dev):
        rs = None
        if self.state is not None:
            if self.masked:                    # the seed as zhusuan.DeviceRNG stores it
                rs = zs.DeviceRNG(dev, seed=self.state[0]).state
                rs[1] = self.state[1]
            else:
                signed = [v - 2 ** 64 if v >= 2 ** 63 else v for v in self.state]
                rs = torch.tensor(signed, dtype=torch.int64, device=dev)
        return dict(seed=self.by_value[0], off=self.by_value[1], rs=rs)


SMALL = Ident("small", 1234, 9)              # both high words zero: the layout of an entry point is read off here
SMALL2 = Ident("small2", 77, 5)
LAYOUT_TOL = 2.0 ** -21                      # the oracle's float32 results against the float64 truth (libm logf: an ulp of 16)
IDS = [
    Ident("zero", 0, 0),
    SMALL,
    Ident("low_words_full", 2 ** 32 - 1, 2 ** 32 - 1),
    Ident("seed_hi_alone", 2 ** 32, 0),
    Ident("torch_default_seed", TORCH_DEFAULT_SEED, 9),
    Ident("call_hi_alone", 1234, 2 ** 32),
    Ident("call_bit63_alone", 0, 2 ** 63 + 5),
    Ident("both_hi_one", 2 ** 32, 2 ** 32),
    Ident("both_hi", 2 ** 63 - 1, 2 ** 63 + 5),
    Ident("seed_full_call_low", 2 ** 64 - 1, 2 ** 32 - 1),
    Ident("all_ones_seed_big_call", 2 ** 64 - 1, 2 ** 63 + 5),
    Ident("state_carry", None, 5, state=(TORCH_DEFAULT_SEED, 2 ** 32 - 2)),           # base + offset crosses 2^32
    Ident("state_masked_seed", None, 5, state=(2 ** 64 - 1, 2 ** 32 - 2), masked=True),
]
BOTH_HI = IDS[8]
SIZES = (1, 3, 4, 5, 7, 8, 1023, 4098)       # vector form, element form, the 8-word tail of PhiloxUniformF


def test_id_matrix_sets_each_high_word_alone_and_together():
    hi = {((i.seed >> 32) != 0, (i.call >> 32) != 0) for i in IDS}
    assert hi == {(False, False), (True, False), (False, True), (True, True)}
    assert IDS[-2].call == 2 ** 32 + 3 and IDS[-1].seed == 2 ** 63 - 1


class Raw3(Raw2):
    def normal_multi(self, shapes, seed=0, off=0, rs=None):
        """zs_normal_sample_logprob_multi with mu = 0, sigma = 1: term t is (K, R, D) with call id off + t; returns the z of
        every term, flat, concatenated."""
        terms = (_hip.MSTerm * len(shapes))()
        keep = []
        for t, (K, R, D) in enumerate(shapes):
            M = R * D
            mu, sg = self.t(np.zeros(M)), self.t(np.ones(M))
            z, lp = self.empty(K, M), self.empty(R, K)
            keep += [mu, sg, z, lp]
            tm = terms[t]
            tm.mu, tm.sigma, tm.eps, tm.z, tm.lp = mu.data_ptr(), sg.data_ptr(), None, z.data_ptr(), lp.data_ptr()
            tm.K, tm.M, tm.D, tm.lp_stride_k, tm.lp_stride_r = K, M, D, 1, K
            tm.offset, tm.sigma_is_logstd = (off + t) & (2 ** 64 - 1), 0
        self.call("zs_normal_sample_logprob_multi_f32", ctypes.byref(terms), len(shapes), seed, rs, None)
        return np.concatenate([keep[4 * t + 2].cpu().numpy().ravel() for t in range(len(shapes))])


@pytest.fixture(scope="module", params=["orc", pytest.param("hip", marks=pytest.mark.gpu)])
def libs(request):
    """(float32, float64) raw-call helpers of the C oracle or of libzs_hip.so"""
    if request.param == "orc":
        k, dev = host_kernel_library(), "cpu"
    else:
        k, dev = _hip.KernelLibrary(_hip.LIB_PATH), "cuda:0"
    return Raw3(k, dev), Raw3(k, dev, torch.float64)


def _oracle():
    return Raw3(host_kernel_library(), "cpu")


# ------------------------------------------------------------------------------------------------ A1
def test_uniform_and_bernoulli_draws_are_the_truth_bit_for_bit(libs):
    r32, r64 = libs
    zero, one = np.zeros(1), np.ones(1)
    p = np.array([0.01, 0.3, 0.5, 0.77, 0.99, 1.0, 0.0])
    for ident in IDS:
        u = truth_u(max(SIZES), ident.call, ident.seed)
        assert np.array_equal(u.astype(np.float32).astype(np.float64), u)          # every value is exact in fp32
        for n in SIZES:
            for raw in (r32, r64):
                tag = (ident.label, n, raw.sfx)
                kw = ident.kw(raw.dev)
                assert np.array_equal(raw.philox_u(n, **kw).astype(np.float64), u[:n]), tag
                pp = raw.t(p).cpu().numpy().astype(np.float64)                     # p as the entry point reads it
                want = (u[:n] < pp[np.arange(n) % p.size]).astype(np.float64)
                assert np.array_equal(raw.bern_sample(p, n, **kw).astype(np.float64), want), tag
                assert not raw.bern_sample(zero, n, **kw).any(), tag               # p = 0 never draws 1
                assert raw.bern_sample(one, n, **kw).all(), tag                    # p = 1 always does
            got = r32.uniform_sample(zero, one, None, n, True, **ident.kw(r32.dev))
            assert np.array_equal(got["out"].astype(np.float64), u[:n]), (ident.label, n)
            assert np.array_equal(got["cache"].astype(np.float64), u[:n]), (ident.label, n)


# ------------------------------------------------------------------------------------------------ A2
def normal_bound(r):
    return ATOL * np.maximum(1.0, r)


def _report(name, err, bound):
    """Print before asserting: the figures of README_rng.md are read from this line."""
    worst = int(np.argmax(err / bound)) if err.size else -1
    print("%-42s n=%-8d max|err|=%.3e  max err/bound=%.4f" % (name, err.size, err.max() if err.size else 0.0,
                                                               (err / bound).max() if err.size else 0.0))
    return worst


def check_normals(name, got, want, r, atol=None):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, name
    assert np.isfinite(got).all(), name
    err = np.abs(got - want)
    bound = normal_bound(r) if atol is None else np.full_like(err, atol)
    worst = _report(name, err, bound)
    assert (err <= bound).all(), (name, worst, float(got[worst]), float(want[worst]), float(r[worst]))


def layout_of(values, table):
    """Index into `table` (a truth stream, or several concatenated) of every element of `values` (an oracle output for a
    small id): the nearest entry, within the oracle's own float32 rounding."""
    order = np.argsort(table)
    st = table[order]
    pos = np.clip(np.searchsorted(st, values), 1, st.size - 1)
    lo, hi = st[pos - 1], st[pos]
    pick = np.where(np.abs(values - lo) <= np.abs(values - hi), pos - 1, pos)
    assert (np.abs(st[pick] - values) <= LAYOUT_TOL * np.maximum(1.0, np.abs(values))).all(), \
        "an oracle draw is not an element of the truth stream"
    idx = order[pick]
    assert np.unique(idx).size == idx.size, "two draws of one launch share a stream element"
    return idx


def logit_table(n, call, seed):
    u = truth_u(n, call, seed)
    return np.log(u) - np.log1p(-u), np.sqrt(-2.0 * np.log(u))


def normal_table(n, call, seed):
    z, r, _ = truth_normal(n, call, seed)
    return z, r


def check_entry(name, raw, run, n_calls, per_call, table=normal_table, atol=None, ids=IDS):
    """`run(raw, **kw)` -> the flat draws of one launch that consumes call ids call .. call + n_calls - 1.  The layout
    (which element is which (call, group, word)) is read off the ORACLE's output at the small id; then, for every id,
    the output of `raw` must be the truth's stream through that layout: changing only the ids changes the device
    output exactly as it changes the oracle's."""
    def tables(ident):
        parts = [table(per_call, (ident.call + j) & (2 ** 64 - 1), ident.seed) for j in range(n_calls)]
        return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    idx = layout_of(run(_oracle(), **SMALL.kw("cpu")).astype(np.float64), tables(SMALL)[0])
    # (two truth values may lie closer together than the oracle's rounding: a second small id confirms every pick)
    again, want2 = run(_oracle(), **SMALL2.kw("cpu")).astype(np.float64), tables(SMALL2)[0][idx]
    assert (np.abs(again - want2) <= LAYOUT_TOL * np.maximum(1.0, np.abs(want2))).all(), "the layout depends on the id"
    for ident in ids:
        want, r = tables(ident)
        check_normals("%s[%s]" % (name, ident.label), run(raw, **ident.kw(raw.dev)), want[idx], r[idx], atol)
    return idx


def test_philox_normal_streams_over_the_id_matrix(libs):
    r32, r64 = libs
    for ident in IDS:
        z, r, _ = truth_normal(max(SIZES), ident.call, ident.seed)
        for n in SIZES:
            check_normals("philox_normal_f32[%s,%d]" % (ident.label, n), r32.philox(n, **ident.kw(r32.dev)), z[:n], r[:n])
            check_normals("philox_normal_f64[%s,%d]" % (ident.label, n), r64.philox(n, **ident.kw(r64.dev)), z[:n], r[:n],
                          ATOL_F64_STREAM)


@pytest.mark.parametrize("K,R,D,kfast", [(3, 5, 4, False), (5, 6, 40, True), (2, 3, 51, False), (1, 7, 1, True)])
def test_normal_sample_draws_over_the_id_matrix(libs, K, R, D, kfast):
    r32, r64 = libs
    mu, sd = np.zeros(R * D), np.ones(R * D)           # z = 0 + 1 * eps: the draw itself, exactly

    def run(raw, **kw):
        return raw.normal_sample(mu, sd, None, K, D, kfast=kfast, **kw)["z"].ravel()
    idx = check_entry("normal_sample_f32", r32, run, 1, K * R * D)
    assert np.array_equal(idx, np.arange(K * R * D))   # flat: element i of z is element i of the stream (include/zs_hip.h)
    check_entry("normal_sample_f64", r64, run, 1, K * R * D, atol=ATOL_F64_SAMPLE)


def _pair_shape(one_launch):
    k = host_kernel_library()
    for K, R, D in PAIR_SHAPES:
        if K * R * D <= 4096 and k.pair_draw_is_one_launch(K, R * D, D) == one_launch:
            return K, R, D
    raise AssertionError("PAIR_SHAPES has no small %s shape" % ("one-launch" if one_launch else "two-launch"))


@pytest.mark.parametrize("one_launch", [True, False], ids=["one_launch", "two_launches"])
def test_pair_draw_over_the_id_matrix(libs, one_launch):
    r32, _ = libs
    K, R, D = _pair_shape(one_launch)
    assert r32.k.pair_draw_is_one_launch(K, R * D, D) == one_launch
    mu, sd = np.zeros(R * D), np.ones(R * D)

    def run(raw, **kw):
        return raw.normal_sample_pair(mu, sd, K, D, **kw)["z"].ravel()
    idx = check_entry("normal_sample_pair_f32", r32, run, 2, K * R * D)
    assert np.array_equal(idx, np.arange(2 * K * R * D))       # half j is the single draw with call id call + j


def test_multi_draw_over_the_id_matrix(libs):
    r32, _ = libs
    shapes = [(3, 5, 4), (2, 1, 51)]
    per_call = max(K * R * D for K, R, D in shapes)

    def run(raw, **kw):
        return raw.normal_multi(shapes, **kw)
    idx = check_entry("normal_sample_multi_f32", r32, run, 2, per_call)
    assert np.array_equal(idx, np.concatenate([np.arange(60), per_call + np.arange(102)]))


def test_logistic_draws_over_the_id_matrix(libs):
    r32, _ = libs
    K, R, D = 3, 9, 7
    loc, sc = np.zeros(R * D), np.ones(R * D)

    def run(raw, **kw):
        return raw.logistic_sample(loc, sc, None, K, D, **kw)["z"].ravel()
    idx = check_entry("logistic_sample_f32", r32, run, 1, K * R * D, table=logit_table)
    assert np.array_equal(idx, np.arange(K * R * D))


# the ids of the samplers' libraries: by value (their rng_state form is pinned against the main library's stream by
# test_mcmc_kernel.py / test_hmc_kernel.py, and the main library's by the tests above) plus the state form with the carry
SAMPLER_IDS = [SMALL, IDS[3], IDS[4], IDS[5], BOTH_HI, IDS[10], IDS[11], IDS[12]]


@pytest.mark.gpu
@pytest.mark.parametrize("sizes", [[5, 7], [8, 12]], ids=["element", "vector"])
def test_mcmc_update_noise_over_the_id_matrix(sizes):
    """zs_mcmc_update_f32: SGHMC_PRE with RESAMPLE_V writes v = sqrt(lr) z, one multiply by the rounded scalar
    (test_mcmc_kernel.py): z is read back as v / c.  Flat element start + i of the launch's stream (include/zs_mcmc.h)."""
    import test_mcmc_kernel as MK
    from zhusuan import _mcmc_hip
    lib = _mcmc_hip.lib(_mcmc_hip.LIB_PATH)
    n = sum(sizes)
    q, g, s, _ = MK.inputs(n, torch.float32, 7)
    c = float(torch.tensor(np.sqrt(MK.HYPER["lr"]), dtype=torch.float64).to(torch.float32))
    for ident in SAMPLER_IDS:
        kw = ident.kw(MK.DEV)
        _, v = MK.run_layout(lib, torch.float32, MK.PRE, MK.RESAMPLE, sizes, None, (q, g, s, torch.zeros(n)), inject=False,
                             seed=kw["seed"], call=kw["off"], rs=kw["rs"])
        z, r, _ = truth_normal(n, ident.call, ident.seed)
        check_normals("mcmc_update_f32[%s]" % ident.label, v.double().numpy() / c, z, r)


@pytest.mark.gpu
@pytest.mark.parametrize("C,rows,shift", [(1, [5, 7], 0), (3, [8, 12], 1)], ids=["element", "vector_shifted"])
def test_hmc_momenta_over_the_id_matrix(C, rows, shift):
    """zs_hmc_move_f32 / _f64 BEGIN returns the momentum it drew in p0 (test_hmc_kernel.py)."""
    import test_hmc_kernel as HK
    from zhusuan import _hmc_hip
    lib = _hmc_hip.lib(_hmc_hip.LIB_PATH)
    n = C * sum(rows)
    for dtype in (HK.F32, HK.F64):
        q, p, g, _ = HK.inputs(n, dtype, 7)
        for ident in SAMPLER_IDS:
            kw = ident.kw(HK.DEV)
            drawn = HK.run_move(lib, dtype, HK.BEGIN, C, rows, shift, (q, p, g, torch.zeros(n, dtype=dtype)), inject=False,
                                seed=kw["seed"], call=kw["off"], rs=kw["rs"])
            z, r, _ = truth_normal(n, ident.call, ident.seed)
            check_normals("hmc_move%s[%s]" % (HK.sfx(dtype), ident.label), drawn[2].double().numpy(), z, r,
                          None if dtype == HK.F32 else ATOL_F64_STREAM)


@pytest.mark.gpu
@pytest.mark.parametrize("C", [3, 257])
def test_hmc_decide_uniforms_over_the_id_matrix(C):
    """zs_hmc_decide_f32 does not return its u: the run that draws must equal, bit for bit, the run that is GIVEN the truth's
    uniforms (exact in fp32), as test_hmc_kernel.py compares it with the main library's stream."""
    import test_hmc_kernel as HK
    from zhusuan import _hmc_hip
    lib = _hmc_hip.lib(_hmc_hip.LIB_PATH)
    k, l0, l1, _ = HK.decide_inputs(C, 5)
    for ident in SAMPLER_IDS:
        kw = ident.kw(HK.DEV)
        drawn = HK.run_decide(lib, HK.F32, C, k, l0, l1, None, HK.state_block(), adapting=1, seed=kw["seed"], call=kw["off"],
                              rs=kw["rs"])
        u = torch.tensor(truth_u(C, ident.call, ident.seed), dtype=torch.float32)
        given = HK.run_decide(lib, HK.F32, C, k, l0, l1, u, HK.state_block(), adapting=1)
        assert all(torch.equal(a, b) for a, b in zip(drawn, given)), ident.label


# ------------------------------------------------------------------------------------------------ A3
def _accuracy_at_scale(name, raw, n, atol):
    ident = BOTH_HI
    got = raw.philox(n, **ident.kw(raw.dev)).astype(np.float64)
    z, r, ur = truth_normal(n, ident.call, ident.seed)
    assert np.isfinite(got).all()
    err = np.abs(got - z)
    bound = normal_bound(r) if atol is None else np.full_like(err, atol)
    us = np.unique(ur)
    pops = {"all": np.ones(n, bool), "r > 4.5": r > 4.5, "|truth| < 1e-3": np.abs(z) < 1e-3,
            "16 smallest u": ur <= us[15], "16 largest u": ur >= us[-16]}
    bad = []
    for key, m in pops.items():
        assert m.any(), "%s: the run does not reach the sub-population %s" % (name, key)
        _report("%s %s" % (name, key), err[m], bound[m])
        if not (err[m] <= bound[m]).all():
            bad.append(key)
    assert r.max() > 5.0 and ur.min() <= 2.0 ** -21       # the tail is really there
    assert not bad, bad


def test_normal_accuracy_at_scale_f32(libs):
    _accuracy_at_scale("A3 f32", libs[0], 1 << 22, None)


def test_normal_accuracy_at_scale_f64(libs):
    _accuracy_at_scale("A3 f64", libs[1], 1 << 20, ATOL_F64_STREAM)


# ------------------------------------------------------------------------------------------------ A4
# The ids of the design statistics, chosen (tools: this file's own truth, on the CPU) so that the TRUTH stream passes every
# statistic below with a wide margin -- KS p >= 0.01, |rho| <= 3 / sqrt(n), bit fractions within 3 standard errors -- which
# test_stream_design[truth] asserts.  The truth's figures for these ids are listed in tests/README_rng.md.
DESIGN_SEED, DESIGN_CALL = TORCH_DEFAULT_SEED, 2 ** 32 + 5
N_DESIGN = 1 << 22
PAIR_DESIGN = (1, 1 << 15, 64)               # (K, R, D): each half of the pair draw holds 2^21 draws, one launch


class TruthSource(object):
    """The numpy truth behind the interface of the raw-call helpers: the design statistics of the stream itself."""
    dev = "cpu"

    def philox(self, n, seed, off, rs=None):
        return truth_normal(n, off, seed)[0]

    def philox_u(self, n, seed, off, rs=None):
        return truth_u(n, off, seed)

    def logistic(self, n, seed, off):
        return logit_table(n, off, seed)[0]

    def pair(self, K, R, D, seed, off):
        return np.stack([truth_normal(K * R * D, off + j, seed)[0] for j in range(2)])


class LibSource(object):
    def __init__(self, raw):
        self.raw, self.dev = raw, raw.dev

    def philox(self, n, seed, off, rs=None):
        return self.raw.philox(n, seed, off).astype(np.float64)

    def philox_u(self, n, seed, off, rs=None):
        return self.raw.philox_u(n, seed, off).astype(np.float64)

    def logistic(self, n, seed, off):
        return self.raw.logistic_sample(np.zeros(1024), np.ones(1024), None, n // 1024, 1024, seed=seed, off=off,
                                        want_lp=False)["z"].ravel().astype(np.float64)

    def pair(self, K, R, D, seed, off):
        assert self.raw.k.pair_draw_is_one_launch(K, R * D, D)
        z = self.raw.normal_sample_pair(np.zeros(R * D), np.ones(R * D), K, D, seed=seed, off=off, want_lp=False)["z"]
        return z.reshape(2, -1).astype(np.float64)


@pytest.fixture(scope="module", params=["truth", "orc", pytest.param("hip", marks=pytest.mark.gpu)])
def source(request):
    if request.param == "truth":
        return TruthSource(), 0.01, 3.0
    k, dev = (host_kernel_library(), "cpu") if request.param == "orc" else (_hip.KernelLibrary(_hip.LIB_PATH), "cuda:0")
    return LibSource(Raw3(k, dev)), 1e-4, 5.0          # p > 1e-4: the threshold of test_distributions.py


def ks_pvalue(x, cdf):
    """The two-sided Kolmogorov-Smirnov test of scipy.stats.kstest(x, cdf) at large n (statistic, then kstwo.sf), without its
    per-call overhead: one sort and one evaluation of the cdf."""
    n = x.size
    f = cdf(np.sort(x))
    i = np.arange(1, n + 1, dtype=np.float64)
    d = max(float((i / n - f).max()), float((f - (i - 1) / n).max()))
    return float(stats.kstwo.sf(d, n))


def _rho(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).mean() / np.sqrt((a * a).mean() * (b * b).mean()))


def design_statistics(src):
    """{name: (kind, value)} with kind 'p' (a KS p-value), 'rho' (a correlation times sqrt(n)) or 'bit' (a mantissa bit's
    fraction minus 1/2 in standard errors)."""
    s, c, n = DESIGN_SEED, DESIGN_CALL, N_DESIGN
    out = {}
    x = src.philox(n, s, c)
    out["KS normal"] = ("p", ks_pvalue(x, special.ndtr))
    for lag in (1, 2, 3, 4, 8):
        out["normal lag %d" % lag] = ("rho", _rho(x[:-lag], x[lag:]) * np.sqrt(n - lag))
    x2 = x * x
    for lag in (1, 2, 3, 4):
        out["squares lag %d" % lag] = ("rho", _rho(x2[:-lag], x2[lag:]) * np.sqrt(n - lag))
    for name, (s2, c2) in {"call c vs c+1": (s, c + 1), "seed s vs s+1": (s + 1, c), "seed s vs s+2^32": (s + 2 ** 32, c)}.items():
        out[name] = ("rho", _rho(x, src.philox(n, s2, c2)) * np.sqrt(n))
    del x2
    halves = src.pair(*PAIR_DESIGN, seed=s, off=c)
    out["pair halves"] = ("rho", _rho(halves[0], halves[1]) * np.sqrt(halves.shape[1]))
    u = src.philox_u(n, s, c)
    out["KS uniform"] = ("p", ks_pvalue(u, lambda v: v))
    for lag in (1, 2, 3, 4, 8):
        out["uniform lag %d" % lag] = ("rho", _rho(u[:-lag], u[lag:]) * np.sqrt(n - lag))
    m = np.round(u * 2.0 ** 23 - 0.5).astype(np.int32)            # the 23 mantissa bits behind u = (m + 0.5) 2^-23
    assert np.array_equal((m + 0.5) * 2.0 ** -23, u) and m.min() >= 0 and m.max() < 2 ** 23
    for b in range(23):
        out["u bit %d" % b] = ("bit", (float(((m >> b) & 1).mean()) - 0.5) / (0.5 / np.sqrt(n)))
    out["KS logistic"] = ("p", ks_pvalue(src.logistic(n, s, c), special.expit))
    return out


def test_stream_design(source):
    src, p_min, k = source
    st = design_statistics(src)
    bad = []
    for name, (kind, v) in st.items():
        print("%-20s %-4s %+.4f" % (name, kind, v))
        if kind == "p":
            ok = v > p_min
        else:                                       # 'rho': |rho| <= k / sqrt(n);  'bit': within k standard errors of 1/2
            ok = abs(v) <= k
        if not ok:
            bad.append((name, v))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ A5
def test_uniform_sample_upper_edge_is_the_references(libs):
    """uniform.py:63-70 of the reference: _sample * (high - low) + low in fp32, two roundings.  With low = 1024, high = 1025 the
    sum rounds up to exactly `high` for the largest u: the reference's behaviour, pinned here so that a change is noticed."""
    r32, _ = libs
    n = 1 << 20
    low, high = np.full(1, 1024.0, np.float32), np.full(1, 1025.0, np.float32)
    ident = BOTH_HI
    got = r32.uniform_sample(low, high, None, n, True, **ident.kw(r32.dev))
    u = truth_u(n, ident.call, ident.seed).astype(np.float32)
    assert np.array_equal(got["cache"], u)
    want = (u * (high - low)).astype(np.float32) + low             # fp32 multiply, fp32 add
    assert want.dtype == np.float32
    assert np.array_equal(got["out"], want)
    assert (got["out"] >= low).all() and (got["out"] <= high).all()
    at_high = int((want == high).sum())
    print("draws equal to high: %d of %d" % (at_high, n))
    assert at_high > 0 and int((got["out"] == high).sum()) == at_high
