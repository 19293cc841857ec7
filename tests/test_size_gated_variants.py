"""The kernel variants that the host dispatch picks from the problem SIZE (tests/README_variants.md): non-temporal stores and
loads beyond the 256 MB Infinity Cache, two particle rows in flight from 400 000 rows, the shared-observation Bernoulli kernels
beyond 32 768 rows, one index-width case beyond 2^31 elements.

Every gate is a pair of cases that differ by one row (CASES): the smallest shape over the gate and its neighbour under it run
the same assertions --
  a. every output element against a float64 evaluation of the reference formula written in plain torch ops on the device
     (normal.py / logistic.py / uniform.py / bernoulli.py incl. its + 1e-8), in chunks of particles.  The
     draws of the sampling kernels come from the flat-stream entry points that test_rng_streams.py pins to the numpy Philox
     (zs_philox_normal_f32 / zs_philox_uniform_f32, same seed and call id); z = mu + sigma * eps bit for bit;
  b. log-densities and gradients within 16 x the distance of a float32 torch restatement from that truth, floored at
     4 * 2^-24 * max|truth| (the rule of test_gradcheck.py section 3; the serial C oracle cannot finish these sizes);
  c. the leading particles of the same problem, run as a problem of its own that lands under the gate, give the same bits;
  d. a second launch into a fresh NaN buffer gives the same bits;
  e. no output element is NaN, a non-finite truth is matched exactly, nothing is left out of a comparison.
test_case_reaches_its_variant proves with torch.profiler which kernel each shape launched; test_case_table_against_the_gates
(not gpu) checks the table's arithmetic against the gate constants.
"""
import functools
import math
import re

import numpy as np
import pytest
import torch

from test_cabi import Raw, hip, orc  # noqa: F401  (the module-scoped raw-ABI fixtures)

F32, F64 = torch.float32, torch.float64
CACHE_BYTES = 1 << 28            # the 256 MB Infinity Cache: every "cannot stay in the cache" gate of the host dispatch
NTL_BYTES = 2.5e9                # zs_bernoulli.hip launch_bwd: non-temporal loads of p
XREUSE_ROWS = 32768              # zs_bernoulli.hip launch_fwd / launch_bwd: rows > 32768 with a shared observation
TWO_ROWS = 400000                # ... rows >= 400000: two particle rows in flight
GRID_CAP = 4096                  # zs_common.h grid_for: the default cap on the workgroups of a grid-stride launch
FEW_ROWS = 2048                  # zs_normal.hip: K * R < 2048 long rows take a workgroup per row

# measure(K, R, D), threshold, strict: the shape is over the gate when measure > threshold (strict) or >= threshold
GATES = {
    "z4": (lambda K, R, D: K * R * D * 4, CACHE_BYTES, True),          # the sample / the gradient, 4 bytes per element
    "z8": (lambda K, R, D: K * R * D * 8, CACHE_BYTES, True),          # given stream + sample (or sample + cache)
    "pair4": (lambda K, R, D: 2 * K * R * D * 4, CACHE_BYTES, True),   # both draws of a pair
    "xreuse": (lambda K, R, D: K * R, XREUSE_ROWS, True),
    "two": (lambda K, R, D: K * R, TWO_ROWS, False),
    "ntl": (lambda K, R, D: K * R * D * 4, NTL_BYTES, True),
    "few": (lambda K, R, D: K * R, FEW_ROWS, False),
    # the caps of grid_for (zs_common.h: 4096 workgroups by default): beyond them the grid-stride loop of a kernel takes a second trip
    "rows4": (lambda K, R, D: K * R, 4 * GRID_CAP, True),                  # a wave per row, four per workgroup
    "rows256": (lambda K, R, D: K * R, 256 * GRID_CAP, True),              # a thread per row
    "tiles6": (lambda K, R, D: (K * R + 5) // 6, 4 * GRID_CAP, True),      # D = 40: six rows per wave pass
    "n256": (lambda K, R, D: K * R * D, 256 * GRID_CAP, True),             # a thread per element
    # zs_locscale.hip launch_rows at D = 10, K-fastest results: tiles of 4 rows x 25 particles, four per workgroup
    "wavetiles": (lambda K, R, D: ((R + 3) // 4) * ((K + 24) // 25), 4 * GRID_CAP, True),
    "rows1": (lambda K, R, D: K * R, 2 * GRID_CAP, True),                  # zs_locscale.hip k_long_rows: a workgroup per row, cap 8192
    "ky": (lambda K, R, D: K, 65535, True),                                # particles beyond the y extent of a grid
}


class Case(object):
    def __init__(self, fam, K, R, D, over, gate, kernel, ksub, **opt):
        self.fam, self.K, self.R, self.D, self.over, self.gate, self.kernel, self.ksub, self.opt = fam, K, R, D, over, gate, kernel, ksub, opt
        tag = "-".join("%s" % (k if v is True else "%s%s" % (k, v)) for k, v in sorted(opt.items()) if v is not False and v is not None)
        self.id = "%s%s-K%d-R%d-D%d-%s-%s" % (fam, "-" + tag if tag else "", K, R, D, gate, "over" if over else "under")

    def __repr__(self):
        return self.id


def pair(fam, K, R, D, gate, k_over, k_under, ksub, **opt):
    """The smallest shape over a gate (R rows per particle) and its neighbour under it (R - 1)."""
    return [Case(fam, K, R, D, True, gate, k_over, ksub, **opt), Case(fam, K, R - 1, D, False, gate, k_under, None, **opt)]


def _cases():
    c = []
    T, F = "true", "false"
    # ---- Normal K1, in-kernel Philox, flat-plane kernel (D = 40: 32 rows per workgroup; 33 555 = 32 * 1048 + 19: ragged last tile)
    for opt in (dict(), dict(nolp=True), dict(logstd=True, rs=True, rowmajor=True)):
        L = F if opt.get("nolp") else T
        c += pair("k1", 50, 33555, 40, "z4", "k_sample_tile<0, %s, true>" % L, "k_sample_tile<0, %s, false>" % L, 25, **opt)
    c += pair("k1pair", 25, 33555, 40, "pair4", "k_sample_tile<0, true, true>", "k_sample_tile<0, true, false>", 12)
    # eps handed in: the given-stream form of the flat-plane kernel, 8 bytes per element
    c += pair("k1", 50, 16778, 40, "z8", "k_logprob_tile<0, true, true>", "k_logprob_tile<0, false, true>", 25, eps=True)
    # D = 100 (D4 = 25: no flat-plane tiling): the row-per-lane-group kernel, eps given and drawn
    c += pair("k1", 50, 13422, 100, "z4", "k_normal_sample_smallrow<true, true, true>", "k_normal_sample_smallrow<true, true, false>", 25, eps=True)
    c += pair("k1", 50, 13422, 100, "z4", "k_normal_sample_smallrow<false, true, true>", "k_normal_sample_smallrow<false, true, false>", 25)
    # long rows (D4 > 64): a workgroup per row below 2048 rows, a wave per row from there on
    c += pair("k1", 8, 256, 260, "few", "k_normal_sample_longrow<false, true, 1>", "k_normal_sample_longrow<false, true, 4>", None)
    # rows that are no multiple of four elements: a wave per row (D >= 8), a thread per row (D < 8); second trip of the grid-stride loop
    c += pair("k1", 50, 328, 10, "rows4", "k_normal_sample_waverow<false>", "k_normal_sample_waverow<false>", 25)
    c += pair("k1", 50, 20972, 3, "rows256", "k_normal_sample_serial<false>", "k_normal_sample_serial<false>", 25)
    c += pair("lp", 50, 328, 10, "rows4", "k_normal_logprob_waverow", "k_normal_logprob_waverow", 25, dist="normal")
    c += pair("lp", 50, 20972, 3, "rows256", "k_normal_logprob_serial", "k_normal_logprob_serial", 25, dist="normal")
    # long rows beyond the cap: a wave per row (K1: k_normal_sample_longrow; K2 with parameters of one plane: k_normal_logprob_rows)
    c += pair("k1", 50, 328, 260, "rows4", "k_normal_sample_longrow<false, true, 1>", "k_normal_sample_longrow<false, true, 1>", 25)
    c += pair("lp", 50, 328, 260, "rows4", "k_normal_logprob_rows", "k_normal_logprob_rows", 25, dist="normal")
    # K2 with full-size parameters (Pm = Ps = N): k_normal_logprob_full, six rows per wave pass at D = 40
    c += pair("lp", 50, 1967, 40, "tiles6", "k_normal_logprob_full", "k_normal_logprob_full", 25, dist="normal", full=True)
    # rows beyond 1024 elements in the generic Logistic path: k_long_rows, a workgroup per row, cap 8192
    c += pair("lp", 50, 164, 1028, "rows1", "k_long_rows<", "k_long_rows<", 25, dist="logistic")
    # ---- given-value log-densities K2 / L2 / U2: flat plane (D = 40, both result layouts) and row tiles (D = 100)
    for d, dist in enumerate(("normal", "logistic", "uniform")):
        for rowmajor in (False, True):
            c += pair("lp", 50, 33555, 40, "z4", "k_logprob_tile<%d, true, false>" % d, "k_logprob_tile<%d, false, false>" % d, 25,
                      dist=dist, rowmajor=rowmajor)
        c += pair("lp", 50, 13422, 100, "z4", "k_logprob_krep<%d, 2, true>" % d, "k_logprob_krep<%d, 4, false>" % d, 25, dist=dist)
    # ---- Logistic L1: drawn (with and without the density) and u handed in
    for opt in (dict(), dict(nolp=True)):
        L = F if opt.get("nolp") else T
        c += pair("l1", 50, 33555, 40, "z4", "k_sample_tile<1, %s, true>" % L, "k_sample_tile<1, %s, false>" % L, 25, **opt)
    c += pair("l1", 50, 16778, 40, "z8", "k_logprob_tile<1, true, true>", "k_logprob_tile<1, false, true>", 25, u=True)
    # rows that are no multiple of four elements: the generic wave-tile kernel of zs_locscale.hip beyond its grid cap
    c += pair("l1", 50, 32769, 10, "wavetiles", "k_wave_rows<", "k_wave_rows<", 25)
    c += pair("lp", 50, 32769, 10, "wavetiles", "k_wave_rows<", "k_wave_rows<", 25, dist="logistic")
    c += pair("lp", 50, 32769, 10, "wavetiles", "k_wave_rows<", "k_wave_rows<", 25, dist="uniform")
    # ---- Uniform U1 (Pl = Ph = 40 R, K = 50 repetitions): N * 4 without the cached draw, N * 8 with it
    for reparam in (0, 1):
        c += pair("u1", 50, 33555, 40, "z4", "k_sample_tile<2, false, true>", "k_sample_tile<2, false, false>", 25, reparam=reparam)
        c += pair("u1", 50, 16778, 40, "z8", "k_sample_tile<2, false, true>", "k_sample_tile<2, false, false>", 25, reparam=reparam, cache=True)
    # ---- Bernoulli forward, D = 256
    for opt, L, W in ((dict(), F, F), (dict(logits=True), T, F), (dict(logits=True, pout=True), T, T)):
        c += pair("bf", 50, 656, 256, "xreuse", "k_bern_logprob_xreuse<%s, %s, 1, true>" % (L, W), "k_bern_logprob_longrow2d<%s, %s>" % (L, W), 49, **opt)
        c += pair("bf", 50, 8000, 256, "two", "k_bern_logprob_xreuse<%s, %s, 2, true>" % (L, W), "k_bern_logprob_xreuse<%s, %s, 1, true>" % (L, W), 49, **opt)
    # K = 51: chunks of 4 particles and a last one of 3 (pick_jc): the second row in flight is switched off in the last round
    c += pair("bf", 51, 7844, 256, "two", "k_bern_logprob_xreuse<false, false, 2, true>", "k_bern_logprob_xreuse<false, false, 1, true>", 50)
    # a per-particle observation (xrows == rows): J = 1, so never the shared-observation kernel, on either side of 32 768 rows
    c += pair("bf", 50, 656, 256, "xreuse", "k_bern_logprob_longrow2d<false, false>", "k_bern_logprob_longrow2d<false, false>", None, xfull=True)
    # grid-stride kernels beyond their grid cap: short rows (D = 40), a thread per row (D = 3), rows beyond 1024 elements (D = 1028)
    c += pair("bf", 50, 1967, 40, "tiles6", "k_bern_logprob_rows<false, false>", "k_bern_logprob_rows<false, false>", 25)
    c += pair("bf", 50, 20972, 3, "rows256", "k_bern_logprob_serial<false>", "k_bern_logprob_serial<false>", 25)
    c += pair("bf", 50, 328, 1028, "rows4", "k_bern_logprob_longrow<false, false>", "k_bern_logprob_longrow<false, false>", 25)
    # ---- Bernoulli backward
    c += pair("bb", 50, 6991, 3, "n256", "k_bern_logprob_bwd_serial<false>", "k_bern_logprob_bwd_serial<false>", 25)
    for opt, L in ((dict(), F), (dict(logits=True), T), (dict(gscale=True), F)):
        c += pair("bb", 50, 656, 256, "xreuse", "k_bern_logprob_bwd_xreuse<%s, false, 1, false>" % L, "k_bern_logprob_bwd_rows<%s, false>" % L, 24, **opt)
        c += pair("bb", 50, 5243, 256, "z4", "k_bern_logprob_bwd_xreuse<%s, true, 1, false>" % L, "k_bern_logprob_bwd_xreuse<%s, false, 1, false>" % L, 49, **opt)
    for opt, L in ((dict(), F), (dict(logits=True, gscale=True), T)):
        c += pair("bb", 50, 8000, 256, "two", "k_bern_logprob_bwd_xreuse<%s, true, 2, false>" % L, "k_bern_logprob_bwd_xreuse<%s, true, 1, false>" % L, 49, **opt)
    c += pair("bb", 51, 7844, 256, "two", "k_bern_logprob_bwd_xreuse<false, true, 2, false>", "k_bern_logprob_bwd_xreuse<false, true, 1, false>", 50)
    c += pair("bb", 50, 33555, 40, "z4", "k_bern_logprob_bwd_rows<false, true>", "k_bern_logprob_bwd_rows<false, false>", 49)
    c += pair("bb", 50, 33555, 40, "z4", "k_bern_logprob_bwd_rows<true, true>", "k_bern_logprob_bwd_rows<true, false>", 49, logits=True)
    c += pair("bb", 50, 656, 256, "xreuse", "k_bern_logprob_bwd_rows<false, false>", "k_bern_logprob_bwd_rows<false, false>", None, xfull=True)
    # 2.5 GB of p: non-temporal loads as well
    c += pair("bb", 50, 12208, 1024, "ntl", "k_bern_logprob_bwd_xreuse<false, true, 2, true>", "k_bern_logprob_bwd_xreuse<false, true, 2, false>", 49, big=True)
    return c


CASES = _cases()
# the one gate on the particle count: grid.y of the wave-per-row kernel holds at most 65 535 particles (zs_bernoulli.hip launch_fwd;
# a shared observation takes the xreuse kernel before that, so the observation here is per particle)
K_CASES = [Case("bf", 65536, 1, 256, True, "ky", "k_bern_logprob_longrow<false, false>", None, xfull=True),
           Case("bf", 65535, 1, 256, False, "ky", "k_bern_logprob_longrow2d<false, false>", None, xfull=True)]
# the index-width shape: 2 148 160 000 elements (> 2^31), byte offsets beyond 2^32 and 2^33 inside p, gp and probs_out
WIDE = dict(K=50, R=54800, D=784, ksub=20)
WIDE_KERNELS = {"fwd": "k_bern_logprob_xreuse<false, false, 2, true>", "fwd_logits_pout": "k_bern_logprob_xreuse<true, true, 2, true>",
                "bwd": "k_bern_logprob_bwd_xreuse<false, true, 2, true>"}


# ---------------------------------------------------------------------------------------------------------------------
# the table against the gate constants (no GPU)
# ---------------------------------------------------------------------------------------------------------------------
def _is_over(c):
    measure, thr, strict = GATES[c.gate]
    v = measure(c.K, c.R, c.D)
    return v > thr if strict else v >= thr


def test_case_table_against_the_gates():
    assert len(CASES) % 2 == 0 and len({c.id for c in CASES}) == len(CASES)
    for o, u in zip(CASES[0::2], CASES[1::2]):
        assert o.over and not u.over
        assert (o.fam, o.K, o.D, o.gate, o.opt) == (u.fam, u.K, u.D, u.gate, u.opt) and o.R - u.R == 1, (o, u)
        assert _is_over(o), o
        assert not _is_over(u), u
        if o.ksub is not None:                                   # the sibling problem lands under the gate
            assert not _is_over(Case(o.fam, o.ksub, o.R, o.D, False, o.gate, "", None)), o
        # every other size gate of the same dispatch function stays on one side for both shapes of the pair
        for g in {"k1": ("z4", "z8"), "l1": ("z4", "z8"), "u1": ("z4", "z8"), "lp": ("z4",), "k1pair": ("pair4",),
                  "bf": ("xreuse", "two"), "bb": ("xreuse", "two", "z4", "ntl")}[o.fam]:
            if g != o.gate and not (o.fam in ("k1", "l1", "u1") and {g, o.gate} == {"z4", "z8"}):
                m, thr, strict = GATES[g]
                a, b = m(o.K, o.R, o.D), m(u.K, u.R, u.D)
                assert (a > thr if strict else a >= thr) == (b > thr if strict else b >= thr), (o, g)
    assert [_is_over(c) for c in K_CASES] == [True, False] and K_CASES[0].K - K_CASES[1].K == 1
    # the cases the issue names, re-derived
    assert 50 * 33555 * 40 == 67110000 > (1 << 26) > 50 * 33554 * 40 and 33555 == 32 * 1048 + 19
    assert 50 * 16778 * 40 * 8 > CACHE_BYTES > 50 * 16777 * 40 * 8
    assert 50 * 13422 * 100 * 4 > CACHE_BYTES > 50 * 13421 * 100 * 4
    assert 50 * 656 > XREUSE_ROWS >= 50 * 655 and 50 * 8000 >= TWO_ROWS > 50 * 7999
    assert 50 * 5243 * 256 * 4 > CACHE_BYTES > 50 * 5242 * 256 * 4
    assert 50 * 12208 * 1024 * 4 > NTL_BYTES > 50 * 12207 * 1024 * 4
    n = WIDE["K"] * WIDE["R"] * WIDE["D"]
    assert n == 2148160000 > (1 << 31) and n * 4 > (1 << 33) and WIDE["ksub"] * WIDE["R"] * WIDE["D"] < (1 << 31)
    # instantiations no argument set reaches (README_variants.md)
    assert TWO_ROWS * 256 * 4 > CACHE_BYTES              # bwd_xreuse<., false, 2, false>: two rows in flight => NT stores
    assert (TWO_ROWS - 1) * 1024 * 4 < NTL_BYTES         # bwd_xreuse<., true, 1, true>: one row in flight => never 2.5 GB
    assert 16384 * 1024 * 4 <= CACHE_BYTES               # bwd_longrow2d<., true>
    assert 32768 * 1024 * 4 <= CACHE_BYTES               # k_iw1_bwd<., true>


# ---------------------------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"
SHARES = {}          # case id -> the largest share of the factor 16 one of its outputs used
_CACHE = {}          # the inputs of ONE shape at a time


def _stops_the_session_on_a_device_fault(test):
    """A HIP error (a launch that failed, an illegal access reported by a later call) ends the pytest session: nothing more is
    started on a device that has faulted.  An assertion that fails is an ordinary failure."""
    @functools.wraps(test)
    def run(*args, **kwargs):
        try:
            return test(*args, **kwargs)
        except AssertionError:
            raise
        except Exception as e:
            if re.search(r"HIP error|hipError|illegal memory|failed with code [1-9]", "%s: %s" % (type(e).__name__, e)):
                pytest.exit("device fault in %s: %s" % (test.__name__, e), returncode=3)
            raise
    return run


def _inputs(key, build):
    if key not in _CACHE:
        _CACHE.clear()
        torch.cuda.empty_cache()
        _CACHE[key] = build()
    return _CACHE[key]


def _gen(*key):
    g = torch.Generator(device=DEV)
    g.manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (1 << 31))
    return g


def _chunk(K, per_particle, budget=1 << 24):
    return max(1, min(K, budget // max(per_particle, 1)))


class Bound(object):
    """Rule b for one output: collects, chunk by chunk, max|got - truth|, max|float32 restatement - truth| and max|truth|."""

    def __init__(self, case_id, name):
        self.case_id, self.name, self.err, self.ref, self.tmax, self.n = case_id, name, 0.0, 0.0, 0.0, 0

    def add(self, got, rest, truth):
        """got / rest: float32; truth: float64; same shape.  A non-finite truth must be matched exactly (and is then left out
        of the distances); a NaN anywhere in `got` fails."""
        assert got.shape == rest.shape == truth.shape
        assert not bool(torch.isnan(got).any()), "%s %s: NaN in the output (an element no thread wrote?)" % (self.case_id, self.name)
        fin = torch.isfinite(truth)
        if not bool(fin.all()):
            assert bool((got[~fin].double() == truth[~fin]).all()), "%s %s: a non-finite truth is not matched exactly" % (self.case_id, self.name)
            got, rest, truth = got[fin], rest[fin], truth[fin]
        if truth.numel() == 0:
            return
        self.n += truth.numel()
        self.err = max(self.err, float((got.double() - truth).abs().max()))
        self.ref = max(self.ref, float((rest.double() - truth).abs().max()))
        self.tmax = max(self.tmax, float(truth.abs().max()))

    def check(self):
        floor = 4 * 2.0 ** -24 * self.tmax
        bound = max(16 * self.ref, floor)
        share = self.err / (bound / 16) if bound > 0 else (0.0 if self.err == 0 else float("inf"))
        SHARES[self.case_id] = max(SHARES.get(self.case_id, 0.0), share)
        print("%s %s: n %d  err %.3e  float32 restatement %.3e  floor %.3e  share %.2f of 16" %
              (self.case_id, self.name, self.n, self.err, self.ref, floor, share))
        assert self.err <= bound, (self.case_id, self.name, self.err, bound)


def _bits_equal(a, b):
    return a.shape == b.shape and bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


def _rows(buf, K, R, rowmajor):
    """[K, R] view of a row result written with (sk, sr) = (R, 1) (row-major) or (1, K) (K-fastest)."""
    return buf.view(K, R) if rowmajor else buf.view(R, K).t()


def _strides(K, R, rowmajor):
    return (R, 1) if rowmajor else (1, K)


def _philox_tail_truth(n, call, seed, groups=4096):
    """float64 (u, normal, r) of the last `groups` Philox groups of flat elements [0, n) (n % 4 == 0) from the numpy Philox of
    test_rng_streams.py, with the Box-Muller layout its _truth() defines."""
    from test_rng_streams import philox_words, _u_of, TWO_PI, U64
    assert n % 4 == 0
    g1 = n // 4
    w = philox_words(np.arange(g1 - groups, g1, dtype=U64), call, seed)
    u = _u_of(w)
    ra, rb = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    a1 = TWO_PI * ((w[:, 1] >> U64(9)).astype(np.float64) * 2.0 ** -23)
    a3 = TWO_PI * ((w[:, 3] >> U64(9)).astype(np.float64) * 2.0 ** -23)
    z = np.stack([ra * np.cos(a1), ra * np.sin(a1), rb * np.cos(a3), rb * np.sin(a3)], axis=1).reshape(-1)
    r = np.stack([ra, ra, rb, rb], axis=1).reshape(-1)
    return u.reshape(-1), z, r


# ---------------------------------------------------------------------------------------------------------------------
# location-scale families: inputs, launches, truths
# ---------------------------------------------------------------------------------------------------------------------
SEED, CALL, BASE = 0x5DEECE66D, 11, 1 << 20


def _ls_inputs(hip, c):
    """Parameters of one [R, D] plane (sigma in [1/e, e]) and the standard draws of K particles: handed-in streams from a seeded
    torch.Generator, in-kernel draws from the flat Philox entry points with the launch's (seed, call id)."""
    K, R, D = c.K, c.R, c.D
    M = R * D
    Kt = 2 * K if c.fam == "k1pair" else K

    def build():
        g = _gen(R, D, 1)
        mu = torch.randn(M, generator=g, device=DEV)
        logstd = torch.rand(M, generator=g, device=DEV) * 2 - 1
        d = dict(mu=mu, logstd=logstd, sigma=torch.exp(logstd))
        call = CALL + (BASE if c.opt.get("rs") else 0)
        if c.fam in ("k1", "k1pair"):
            if c.opt.get("eps"):
                d["eps"] = torch.randn(K * M, generator=g, device=DEV)
            else:
                d["eps"] = hip.empty(Kt * M)
                for j in range(Kt // K):          # the second draw of a pair: call id + 1, counters from its own first particle
                    hip.call("zs_philox_normal_f32", d["eps"][j * K * M:(j + 1) * K * M], K * M, SEED, call + j, None)
        elif c.fam == "l1":
            if c.opt.get("u"):
                d["u"] = torch.rand(K * M, generator=g, device=DEV).clamp_(1e-7, 1 - 1e-7)
            else:
                d["u"] = hip.empty(K * M)
                hip.call("zs_philox_uniform_f32", d["u"], K * M, SEED, CALL, None)
        elif c.fam == "u1":
            d["width"] = torch.rand(M, generator=g, device=DEV) + 0.5
            d["high"] = mu + d["width"]
            d["u"] = hip.empty(K * M)
            hip.call("zs_philox_uniform_f32", d["u"], K * M, SEED, CALL, None)
        elif c.fam == "lp":
            x = torch.randn(K * M, generator=g, device=DEV)
            if c.opt["dist"] == "uniform":
                d["width"] = torch.rand(M, generator=g, device=DEV) + 0.5
                d["high"] = mu + d["width"]
                x = (mu.view(1, M) + d["width"].view(1, M) * torch.rand(K, M, generator=g, device=DEV)).view(-1)
                # a handful of values outside the support, at both bounds: rows whose truth is -inf
                x[7], x[K * M - 3], x[(K // 2) * M + 5] = mu[7] - 1.0, d["high"][M - 3], d["high"][5] + 0.5
            else:
                x = mu.repeat(K) + d["sigma"].repeat(K) * x * 1.5
            d["x"] = x
            if c.opt.get("full"):
                d["mu_full"], d["sigma_full"] = mu.repeat(K), d["sigma"].repeat(K)
        return d
    return _inputs(("ls", c.fam, K, R, D, tuple(sorted(c.opt.items()))), build)


def _ls_prepare(hip, c, inp, K):
    """Allocates NaN-filled outputs for the first K particles of the case and returns (launch, outputs)."""
    R, D = c.R, c.D
    M = R * D
    o = c.opt
    rowmajor = bool(o.get("rowmajor"))
    Kt = 2 * K if c.fam == "k1pair" else K
    sk, sr = _strides(Kt, R, rowmajor)
    out = {}
    if c.fam in ("k1", "k1pair", "l1"):
        out["z"] = hip.empty(Kt * M)
        lp = None if o.get("nolp") else hip.empty(Kt * R)
        if lp is not None:
            out["lp"] = lp
        rs = used = None
        if o.get("rs"):
            rs = torch.tensor([SEED, BASE], dtype=torch.int64, device=DEV)
            used = out["used"] = torch.zeros(2, dtype=torch.int64, device=DEV)
        seed = 1 if rs is not None else SEED        # (ignored by the kernel when rng_state is given)
        if c.fam == "k1":
            sig = inp["logstd"] if o.get("logstd") else inp["sigma"]
            eps = inp["eps"][:K * M] if o.get("eps") else None
            args = ("zs_normal_sample_logprob_f32", inp["mu"], sig, eps, seed, CALL, rs, out["z"], lp, K, M, D, sk, sr,
                    int(bool(o.get("logstd"))), used)
        elif c.fam == "k1pair":
            args = ("zs_normal_sample_logprob_pair_f32", inp["mu"], inp["sigma"], seed, CALL, rs, out["z"], lp, K, M, D, sk, sr, 0, used)
        else:
            u = inp["u"][:K * M] if o.get("u") else None
            args = ("zs_logistic_sample_logprob_f32", inp["mu"], inp["sigma"], u, seed, CALL, rs, out["z"], lp, K, M, D, sk, sr, used)
    elif c.fam == "u1":
        out["out"] = hip.empty(K * M)
        cache = None
        if o.get("cache"):
            cache = out["cache"] = hip.empty(K * M)
        args = ("zs_uniform_sample_f32", inp["mu"], M, inp["high"], M, None, SEED, CALL, None, out["out"], cache, K * M, int(o["reparam"]))
    else:
        out["lp"] = hip.empty(K * R)
        name = {"normal": "zs_normal_logprob_f32", "logistic": "zs_logistic_logprob_f32", "uniform": "zs_uniform_logprob_f32"}[o["dist"]]
        b = inp["high"] if o["dist"] == "uniform" else inp["sigma"]
        if o.get("full"):          # parameters of the full problem's size (the leading K particles' share of them)
            args = (name, inp["x"][:K * M], K * M, inp["mu_full"][:K * M], K * M, inp["sigma_full"][:K * M], K * M, out["lp"], K, R, D, sk, sr, 0)
        else:
            args = (name, inp["x"][:K * M], K * M, inp["mu"], M, b, M, out["lp"], K, R, D, sk, sr) + ((0,) if o["dist"] == "normal" else ())
    return (lambda: hip.call(*args)), out


HALF_LOG_2PI = 0.5 * math.log(2 * math.pi)


def _normal_terms(x, mu, sigma):
    return (-HALF_LOG_2PI - torch.log(sigma) - 0.5 * ((x - mu) / sigma) ** 2).sum(-1)            # normal.py:109-126


def _logistic_terms(x, mu, s):
    t = (x - mu) / s
    return (-t - 2 * torch.nn.functional.softplus(-t) - torch.log(s)).sum(-1)                    # logistic.py:81-82


def _logistic_fresh_terms(eps, s):
    return (-eps - 2 * torch.nn.functional.softplus(-eps) - torch.log(s)).sum(-1)                 # t == eps for the fresh sample


def _uniform_terms(x, low, high):
    inside = ((low <= x) & (high > x)).to(x.dtype)
    return (torch.log(inside) - torch.log(high - low)).sum(-1)                                   # uniform.py:72-85


def _ls_check(hip, c, inp, out, K):
    """Checks a, b and e of the location-scale cases on the outputs of a launch with K particles."""
    R, D = c.R, c.D
    M = R * D
    o = c.opt
    rowmajor = bool(o.get("rowmajor"))
    halves = 2 if c.fam == "k1pair" else 1
    Kt = halves * K
    kc = _chunk(K, M)
    mu, sigma = inp["mu"], inp["sigma"]
    for name, t in out.items():
        assert not bool(torch.isnan(t).any()) if t.is_floating_point() else True, (c.id, name)
    if "used" in out:
        assert out["used"].cpu().tolist() == [SEED, BASE + CALL]
    if c.fam in ("k1", "k1pair"):
        z = out["z"].view(Kt, M)
        lp = _rows(out["lp"], Kt, R, rowmajor) if "lp" in out else None
        b = Bound(c.id, "lp")
        s64 = torch.exp(inp["logstd"].double()) if o.get("logstd") else sigma.double()
        s32 = torch.exp(inp["logstd"]) if o.get("logstd") else sigma
        for h in range(halves):
            eps = inp["eps"][h * (len(inp["eps"]) // halves):].view(-1, M)            # this draw's particles
            for k0 in range(0, K, kc):
                k1 = min(K, k0 + kc)
                zz, e = z[h * K + k0:h * K + k1], eps[k0:k1]
                if o.get("logstd"):      # the tolerances of test_cabi.py::test_hip_normal_logstd_form
                    want = mu.double() + s64 * e.double()
                    assert bool(((zz.double() - want).abs() <= 2e-6 + 2e-6 * want.abs()).all()), (c.id, "z", k0)
                else:                    # z = mu + sigma * eps with two roundings, bit for bit
                    prod = sigma * e
                    assert _bits_equal(zz, mu + prod), (c.id, "z is not mu + sigma * eps bit for bit", h, k0)
                if lp is not None:
                    b.add(lp[h * K + k0:h * K + k1].contiguous(), _normal_terms(zz.view(-1, R, D), mu.view(R, D), s32.view(R, D)),
                          _normal_terms(zz.double().view(-1, R, D), mu.double().view(R, D), s64.view(R, D)))
        if lp is not None:
            b.check()
    elif c.fam == "l1":
        z = out["z"].view(K, M)
        lp = _rows(out["lp"], K, R, rowmajor) if "lp" in out else None
        b = Bound(c.id, "lp")
        u = inp["u"].view(-1, M)
        atol = (2e-6 if o.get("u") else 4e-6) * float(sigma.max())          # test_locscale.py::test_hip_logistic_sample_and_backward
        for k0 in range(0, K, kc):
            k1 = min(K, k0 + kc)
            u64 = u[k0:k1].double()
            e64 = torch.log(u64) - torch.log1p(-u64)                        # logistic.py:64-65
            want = mu.double() + sigma.double() * e64
            assert bool(((z[k0:k1].double() - want).abs() <= atol + 1e-5 * want.abs()).all()), (c.id, "z", k0)
            if lp is not None:
                e32 = torch.log(u[k0:k1]) - torch.log1p(-u[k0:k1])
                b.add(lp[k0:k1].contiguous(), _logistic_fresh_terms(e32.view(-1, R, D), sigma.view(R, D)),
                      _logistic_fresh_terms(e64.view(-1, R, D), sigma.double().view(R, D)))
        if lp is not None:
            b.check()
    elif c.fam == "u1":
        u, width = inp["u"].view(-1, M), inp["high"] - mu                    # (high - low) rounded once, as the kernel forms it
        for k0 in range(0, K, kc):
            k1 = min(K, k0 + kc)
            cch = u[k0:k1] if o["reparam"] else mu + u[k0:k1] * width        # uniform.py:63-70, two roundings each: bit for bit
            prod = cch * width
            assert _bits_equal(out["out"].view(K, M)[k0:k1], mu + prod), (c.id, "out", k0)
            if "cache" in out:
                assert _bits_equal(out["cache"].view(K, M)[k0:k1], cch.expand(k1 - k0, M).contiguous()), (c.id, "cache", k0)
    else:
        lp = _rows(out["lp"], K, R, rowmajor)
        b = Bound(c.id, "lp")
        x = inp["x"].view(-1, R, D)
        f = {"normal": _normal_terms, "logistic": _logistic_terms, "uniform": _uniform_terms}[o["dist"]]
        second = inp["high"] if o["dist"] == "uniform" else sigma
        for k0 in range(0, K, kc):
            k1 = min(K, k0 + kc)
            b.add(lp[k0:k1].contiguous(), f(x[k0:k1], mu.view(R, D), second.view(R, D)),
                  f(x[k0:k1].double(), mu.double().view(R, D), second.double().view(R, D)))
        b.check()
        if o["dist"] == "uniform":
            assert int(torch.isinf(lp).sum()) >= 1                          # the rows with a value outside the support


def _ls_sibling(c, out, sub, K, Ks):
    """Check c: the first Ks particles, run as their own problem, give the bits of the K-particle launch."""
    R, M = c.R, c.R * c.D
    rowmajor = bool(c.opt.get("rowmajor"))
    halves = 2 if c.fam == "k1pair" else 1
    for name in out:
        if name == "used":
            continue
        per = R if name == "lp" else M
        for h in range(halves):
            if name == "lp":
                a = _rows(out[name], halves * K, R, rowmajor)[h * K:h * K + Ks]
                b = _rows(sub[name], halves * Ks, R, rowmajor)[h * Ks:(h + 1) * Ks]
            else:
                a, b = out[name].view(halves * K, per)[h * K:h * K + Ks], sub[name].view(halves * Ks, per)[h * Ks:(h + 1) * Ks]
            assert _bits_equal(a.contiguous(), b.contiguous()), (c.id, name, "the %d leading particles differ from the sub-problem's" % Ks)


LS_CASES = [c for c in CASES if c.fam in ("k1", "k1pair", "l1", "u1", "lp")]


@pytest.mark.gpu
@pytest.mark.parametrize("c", LS_CASES, ids=[c.id for c in LS_CASES])
@_stops_the_session_on_a_device_fault
def test_location_scale_variants(hip, c):
    inp = _ls_inputs(hip, c)
    launch, out = _ls_prepare(hip, c, inp, c.K)
    launch()
    _ls_check(hip, c, inp, out, c.K)
    launch2, out2 = _ls_prepare(hip, c, inp, c.K)                  # d. a second launch into fresh NaN buffers
    launch2()
    for name in out:
        assert _bits_equal(out[name], out2[name]) if out[name].is_floating_point() else bool(torch.equal(out[name], out2[name])), (c.id, name, "second launch")
    del out2
    if c.ksub is not None:
        launch3, sub = _ls_prepare(hip, c, inp, c.ksub)
        launch3()
        _ls_sibling(c, out, sub, c.K, c.ksub)


@pytest.mark.gpu
@_stops_the_session_on_a_device_fault
def test_last_philox_groups_of_the_largest_draws_against_numpy(hip):
    """The last 4096 Philox groups of the largest Normal draw (K = 50, R = 33 555, D = 40: 16 777 500 groups) and of the Uniform
    draw of that size against the numpy Philox of test_rng_streams.py -- the samples themselves, not only the flat
    stream they are compared with elsewhere in this file."""
    from test_rng_streams import ATOL
    c = next(c for c in CASES if c.fam == "k1" and c.over and not c.opt)
    inp = _ls_inputs(hip, c)
    launch, out = _ls_prepare(hip, c, inp, c.K)
    launch()
    M, n, T = c.R * c.D, c.K * c.R * c.D, 4 * 4096
    u, zn, r = _philox_tail_truth(n, CALL, SEED)
    m = torch.arange(n - T, n, device=DEV) % M
    mu, sg = inp["mu"][m].double().cpu().numpy(), inp["sigma"][m].double().cpu().numpy()
    got = out["z"][n - T:].double().cpu().numpy()
    want = mu + sg * zn
    assert np.all(np.abs(got - want) <= sg * ATOL * np.maximum(1.0, r) + 2.0 ** -22 * np.abs(want))
    eps = inp["eps"][n - T:].double().cpu().numpy()
    assert np.all(np.abs(eps - zn) <= ATOL * np.maximum(1.0, r))
    c = next(c for c in CASES if c.fam == "u1" and c.over and c.opt.get("reparam") == 1 and not c.opt.get("cache"))
    inp = _ls_inputs(hip, c)
    launch, out = _ls_prepare(hip, c, inp, c.K)
    launch()
    width = (inp["high"] - inp["mu"])[m]
    prod = inp["u"][n - T:] * width
    assert np.array_equal(inp["u"][n - T:].cpu().numpy(), u.astype(np.float32))                # u01 is exact in float32
    assert _bits_equal(out["out"][n - T:], inp["mu"][m] + prod)
    assert np.array_equal(out["out"][n - T:].cpu().numpy(),
                          (inp["mu"][m].cpu().numpy() + (u.astype(np.float32) * width.cpu().numpy()).astype(np.float32)).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------------
# Bernoulli
# ---------------------------------------------------------------------------------------------------------------------
def _bern_inputs(K, R, D, logits, xfull, need_glp):
    N, rows = K * R * D, K * R

    def build():
        g = _gen(K, R, D, 2)
        p = torch.rand(N, generator=g, device=DEV)
        if logits:
            p.mul_(12).sub_(6)
        # probabilities of exactly 0 and 1 (logits: +-30, sigmoid(30) == 1 in float32) at a handful of positions, inside and
        # beyond the leading particles of the sibling problems
        lo, hi = (-30.0, 30.0) if logits else (0.0, 1.0)
        for i, v in ((0, lo), (1, hi), (N // 3, lo), (N // 2 + 1, hi), (N - 2, lo), (N - 1, hi), (R * D + 17, lo), (2 * R * D - 5, hi)):
            p[i] = v
        Px = N if xfull else R * D
        x = (torch.rand(Px, generator=g, device=DEV) < 0.5).float()
        xr = x.view(-1, D)
        xr[1::2] = torch.rand(xr[1::2].shape, generator=g, device=DEV)       # every other observation row is fractional
        d = dict(p=p, x=x)
        d["glp"] = torch.randn(R, K, generator=g, device=DEV)                # K-fastest: element (k, r) at r * K + k
        d["gscale"] = torch.rand(R, generator=g, device=DEV) + 0.5
        return d
    return _inputs(("bern", K, R, D, logits, xfull), build)


BERN_EPS = 1e-8


def _bern_p(pl, logits):
    return torch.sigmoid(pl) if logits else pl


def _bern_lp(pl, x, logits):
    p = _bern_p(pl, logits)
    return (x * torch.log(p + BERN_EPS) + (1 - x) * torch.log((1 - p) + BERN_EPS)).sum(-1)      # bernoulli.py:84-95


def _bern_gp(pl, x, g, logits):
    p = _bern_p(pl, logits)
    d = x / (p + BERN_EPS) - (1 - x) / ((1 - p) + BERN_EPS)
    if logits:
        d = d * p * (1 - p)
    return g.unsqueeze(-1) * d


def _bern_prepare(hip, c, inp, K, wide_p=None):
    R, D, o = c.R, c.D, c.opt
    N = K * R * D
    Px = N if o.get("xfull") else R * D
    x = inp["x"][:Px]
    p = inp["p"][:N]
    out = {}
    if c.fam == "bf":
        out["lp"] = hip.empty(K * R)
        if o.get("logits"):
            po = None
            if o.get("pout"):
                po = out["pout"] = hip.empty(N)
            args = ("zs_bernoulli_logits_logprob_f32", p, x, Px, out["lp"], po, K, R, D, 1, K)
        else:
            args = ("zs_bernoulli_logprob_f32", p, x, Px, out["lp"], K, R, D, 1, K)
    else:
        out["gp"] = hip.empty(N)
        glp = inp["glp"] if K == inp["glp"].shape[1] else inp["glp"][:, :K].contiguous()
        if o.get("gscale"):
            # the objective's incoming gradient as a device vector (IW1's backward without the variational node: launch_bwd with gscale)
            args = ("zs_bernoulli_iw_objective_bwd_f32", p, int(bool(o.get("logits"))), x, Px, K, R, D, glp, inp["gscale"], 1, out["gp"],
                    None, None, None, 0, 0, None, None)
        else:
            name = "zs_bernoulli_logits_logprob_bwd_f32" if o.get("logits") else "zs_bernoulli_logprob_bwd_f32"
            args = (name, p, x, Px, glp, 1, K, out["gp"], K, R, D)
        out["_glp"] = glp
    return (lambda: hip.call(*args)), out


# Rule b on the Bernoulli gradient, one class of elements per decade of |truth| (the last one: the handful at a probability of
# exactly 0 or 1, up to 1e8 |g|), each with its own max|truth| and its own float32-restatement distance.  p is uniform on
# [0, 1), so |gradient| ~ 1 / p is heavy-tailed: one bound over the tensor (floor 4 * 2^-24 * 1e8 ~ 2e1), or over everything below
# 1e4 (~ 1e-2 absolute), would leave the typical element, of size 1 - 10, all but unchecked.  Within a decade the floor is at most
# 2.4e-6 relative to the element.  Every element falls into exactly one class.
GP_CLASSES = (0.0, 1.0, 1e1, 1e2, 1e3, 1e4, float("inf"))


def _bern_check(c, inp, out, K):
    R, D, o = c.R, c.D, c.opt
    logits, xfull = bool(o.get("logits")), bool(o.get("xfull"))
    M = R * D
    p = inp["p"][:K * M].view(K, R, D)
    x = inp["x"][:K * M].view(K, R, D) if xfull else inp["x"].view(1, R, D)
    kc = _chunk(K, M)
    if c.fam == "bf":
        lp = out["lp"].view(R, K).t()
        b, bp = Bound(c.id, "lp"), Bound(c.id, "probs_out")
        for k0 in range(0, K, kc):
            k1 = min(K, k0 + kc)
            xs = x[k0:k1] if xfull else x
            b.add(lp[k0:k1].contiguous(), _bern_lp(p[k0:k1], xs, logits), _bern_lp(p[k0:k1].double(), xs.double(), logits))
            if "pout" in out:
                bp.add(out["pout"].view(K, R, D)[k0:k1], torch.sigmoid(p[k0:k1]), torch.sigmoid(p[k0:k1].double()))
        b.check()
        if "pout" in out:
            bp.check()
    else:
        gp = out["gp"].view(K, R, D)
        g = out["_glp"].t()                                       # [K, R]
        if o.get("gscale"):
            g = g * inp["gscale"].view(1, R)                      # one rounding, as the kernel forms glp * gscale
        bounds = [Bound(c.id, "gp, %g <= |truth| < %g" % (lo, hi)) for lo, hi in zip(GP_CLASSES[:-1], GP_CLASSES[1:])]
        for k0 in range(0, K, kc):
            k1 = min(K, k0 + kc)
            xs = x[k0:k1] if xfull else x
            truth = _bern_gp(p[k0:k1].double(), xs.double(), g[k0:k1].double(), logits)
            rest = _bern_gp(p[k0:k1], xs, g[k0:k1], logits)
            got = gp[k0:k1]
            assert not bool(torch.isnan(got).any()), (c.id, "NaN in gp")
            mag = truth.abs()
            for b, lo, hi in zip(bounds, GP_CLASSES[:-1], GP_CLASSES[1:]):
                sel = (mag >= lo) & (mag < hi)
                if bool(sel.any()):
                    b.add(got[sel], rest[sel], truth[sel])
        assert sum(b.n for b in bounds) == K * M
        for b in bounds:
            if b.n:
                b.check()


def _packed_row_sum(K, R, D, o):
    """Whether the forward launch of (K, R, D) adds packed pairs (bern_piece_acc): only k_bern_logprob_xreuse<true, ., 1, .>, the logits
    form with ONE row in flight (zs_bernoulli.hip launch_fwd: shared observation, 256 <= D <= 1024, 32768 < rows < 400000)."""
    return bool(o.get("logits")) and not o.get("xfull") and D % 4 == 0 and 64 <= D // 4 <= 256 and K >= 2 and XREUSE_ROWS < K * R < TWO_ROWS


def _bern_sibling(c, out, sub, K, Ks):
    R, D, o = c.R, c.D, c.opt
    for name in out:
        if name.startswith("_"):
            continue
        if name == "lp":
            if _packed_row_sum(K, R, D, o) != _packed_row_sum(Ks, R, D, o):
                # a real difference in the arithmetic: the one-row logits form of k_bern_logprob_xreuse adds packed pairs
                # (bern_piece_acc), the two-row form and longrow2d add scalar terms (bern_row_terms) -- tolerance gate only
                continue
            a, b = out["lp"].view(R, K)[:, :Ks].contiguous(), sub["lp"].view(R, Ks)
        else:
            a, b = out[name][:Ks * R * D], sub[name]
        assert _bits_equal(a, b), (c.id, name, "the %d leading particles differ from the sub-problem's" % Ks)


BERN_CASES = [c for c in CASES + K_CASES if c.fam in ("bf", "bb")]


@pytest.mark.gpu
@pytest.mark.parametrize("c", BERN_CASES, ids=[c.id for c in BERN_CASES])
@_stops_the_session_on_a_device_fault
def test_bernoulli_variants(hip, c):
    inp = _bern_inputs(c.K, c.R, c.D, bool(c.opt.get("logits")), bool(c.opt.get("xfull")), c.fam == "bb")
    launch, out = _bern_prepare(hip, c, inp, c.K)
    launch()
    _bern_check(c, inp, out, c.K)
    launch2, out2 = _bern_prepare(hip, c, inp, c.K)
    launch2()
    for name in out:
        assert _bits_equal(out[name], out2[name]), (c.id, name, "second launch")
    del out2
    if c.ksub is not None:
        launch3, sub = _bern_prepare(hip, c, inp, c.ksub)
        launch3()
        _bern_sibling(c, out, sub, c.K, c.ksub)


def _checksum(t):
    """Two position-dependent 64-bit sums over the bits of a float32 tensor (determinism of a result too large to keep twice)."""
    v = t.view(torch.int32)
    s0 = s1 = 0
    step = 1 << 27
    for i in range(0, v.numel(), step):
        w = v[i:i + step].long()
        s0 += int(w.sum())
        s1 += int((w * (torch.arange(w.numel(), device=w.device) % 8191 + 1)).sum()) + (i // step) * int(w.sum() % 1000003)
    return s0, s1


@pytest.mark.gpu
@_stops_the_session_on_a_device_fault
def test_bernoulli_beyond_2_31_elements(hip):
    """D = 784, K = 50, R = 54 800: 2 148 160 000 elements -- element indices beyond 2^31, byte offsets beyond 2^33 -- through the
    kernels the sweeps run at 13 - 27 GB: forward (probs; logits with probs_out) and backward, every element against float64."""
    K, R, D, Ks = WIDE["K"], WIDE["R"], WIDE["D"], WIDE["ksub"]
    torch.cuda.synchronize()
    for fam, opt in (("bf", {}), ("bb", {}), ("bf", dict(logits=True, pout=True))):
        c = Case(fam, K, R, D, True, "two", "", Ks, **opt)
        c.id = "wide-" + c.id
        inp = _bern_inputs(K, R, D, bool(opt.get("logits")), False, fam == "bb")
        launch, out = _bern_prepare(hip, c, inp, K)
        launch()
        _bern_check(c, inp, out, K)
        launch3, sub = _bern_prepare(hip, c, inp, Ks)
        launch3()
        _bern_sibling(c, out, sub, K, Ks)
        del sub, launch3
        big = "gp" if fam == "bb" else ("pout" if "pout" in out else None)
        lp0 = out["lp"].clone() if "lp" in out else None
        sums = _checksum(out[big]) if big else None
        del out, launch                                            # 8.6 GB: p, the result and its repeat do not fit 24 GB together
        torch.cuda.empty_cache()
        launch2, out2 = _bern_prepare(hip, c, inp, K)
        launch2()
        if lp0 is not None:
            assert _bits_equal(lp0, out2["lp"])
        if big:
            assert _checksum(out2[big]) == sums, (c.id, "second launch")
        del out2, launch2
    _CACHE.clear()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# which kernel ran
# ---------------------------------------------------------------------------------------------------------------------
def _kernels_of(launch):
    """Names of the device kernels one launch started, from torch.profiler; fails when the profiler reports no device event."""
    from torch.profiler import profile, ProfilerActivity
    probe = torch.zeros(8, device=DEV)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        probe.add_(1.0)                  # a torch kernel that must show up: no device events at all => the claim is unproven
        launch()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if (e.device_time if hasattr(e, "device_time") else e.cuda_time) > 0]
    assert names, "torch.profiler reported no device events in this process: which variant ran is unproven"
    ours = [n for n in names if "k_" in n and ("zs::" in n or "(anonymous namespace)::" in n) and "at::" not in n]
    return ours, names


def _prepare_any(hip, c):
    if c.fam in ("bf", "bb"):
        inp = _bern_inputs(c.K, c.R, c.D, bool(c.opt.get("logits")), bool(c.opt.get("xfull")), c.fam == "bb")
        return _bern_prepare(hip, c, inp, c.K)
    return _ls_prepare(hip, c, _ls_inputs(hip, c), c.K)


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES + K_CASES, ids=[c.id for c in CASES + K_CASES])
@_stops_the_session_on_a_device_fault
def test_case_reaches_its_variant(hip, c):
    launch, out = _prepare_any(hip, c)
    ours, names = _kernels_of(launch)
    assert len(ours) == 1, (c.id, ours, names)
    want = c.kernel if c.kernel.endswith("<") else c.kernel + "("          # ("<": a functor-templated kernel, named without its arguments)
    assert want in ours[0], (c.id, "expected", c.kernel, "ran", ours[0])
    print("%s -> %s" % (c.id, ours[0][:ours[0].index(c.kernel) + len(c.kernel)]))


@pytest.mark.gpu
@_stops_the_session_on_a_device_fault
def test_wide_case_reaches_its_variants(hip):
    K, R, D = WIDE["K"], WIDE["R"], WIDE["D"]
    for key, fam, opt in (("fwd", "bf", {}), ("bwd", "bb", {}), ("fwd_logits_pout", "bf", dict(logits=True, pout=True))):
        c = Case(fam, K, R, D, True, "two", WIDE_KERNELS[key], None, **opt)
        launch, out = _prepare_any(hip, c)
        ours, names = _kernels_of(launch)
        assert len(ours) == 1 and c.kernel + "(" in ours[0], (key, ours, names)
        del launch, out
    _CACHE.clear()
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------
# the lane-group bucket of zs_iw_reduce that no earlier test reaches: B >= 16384 datapoints on 8 lanes each, 17 <= K <= 32
# (ni = ceil(K / 8) in (2, 4]: k_iw_reduce_group<8, 4>; test_cabi.py::test_hip_iw_reduce_lane_groups runs <8, 2>, <8, 7>, <8, 8> and
# the three 16-lane buckets)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B,K", [(16384, 17), (16385, 24), (20000, 32)])
@_stops_the_session_on_a_device_fault
def test_iw_reduce_lane_group_bucket_of_four(hip, orc, B, K):
    from test_cabi import _check_iw_reduce
    for spread in (1.0, 30.0):
        _check_iw_reduce(hip, orc, B, K, spread)
    lp = torch.randn(B, K, generator=_gen(B, K, 3), device=DEV)
    lq = lp * 0.5
    outs = [hip.empty(B), hip.empty(B), hip.empty(B, K), hip.empty(B, K)]
    ours, names = _kernels_of(lambda: hip.call("zs_iw_reduce_f32", lp, K, lq, K, B, K, 1, *outs))
    assert len(ours) == 1 and "k_iw_reduce_group<8, 4>(" in ours[0], (ours, names)


# ---------------------------------------------------------------------------------------------------------------------
# two more size gates outside the four distribution families (README_variants.md): MS1's backward gives every element a
# thread of its own from 65 536 elements per node (zs_logjoint.hip ms_build: ks = 1, else up to 16 K-slices), and A1 caps its
# grid at 1024 instead of 256 workgroups beyond 2^24 parameters (zs_adam.hip)
# ---------------------------------------------------------------------------------------------------------------------
MS_GATE, ADAM_GATE = 65536, 1 << 24


def test_ms1_and_adam_shapes_against_their_gates():
    assert 8192 * 8 >= MS_GATE > 8191 * 8 and (1 << 24) + 4 > ADAM_GATE >= (1 << 24)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [8192, 8191], ids=["M65536-over", "M65528-under"])
@_stops_the_session_on_a_device_fault
def test_multi_node_backward_across_65536_elements(hip, R):
    from test_logjoint import Raw as RawLJ
    K, D = 4, 8
    M = R * D
    g = _gen(K, R, D, 4)
    sigma = torch.exp(torch.rand(M, generator=g, device=DEV) * 2 - 1).cpu().numpy()
    eps, gz = (torch.randn(K, M, generator=g, device=DEV).cpu().numpy() for _ in range(2))
    glp = torch.randn(K, R, generator=g, device=DEV).cpu().numpy()
    node = dict(sigma=sigma, eps=eps.ravel(), gz=gz.ravel(), glp=glp.ravel(), K=K, D=D)
    raw = RawLJ(hip.k, DEV)
    (gmu, gs), = raw.ms_bwd([node])
    (gmu2, gs2), = raw.ms_bwd([node])
    assert np.array_equal(gmu, gmu2) and np.array_equal(gs, gs2)

    def formula(dt):          # zs_hip.h, backward of K1: gmu = sum_k gz, gsigma = sum_k gz * eps - (sum_k glp) / sigma
        a, b = np.zeros(M, dt), np.zeros(M, dt)
        for k in range(K):
            a += gz[k].astype(dt)
            b += gz[k].astype(dt) * eps[k].astype(dt)
        return a, b - np.repeat(glp.astype(dt).sum(0), D) / sigma.astype(dt)
    cid = "ms1-bwd-K%d-R%d-D%d" % (K, R, D)
    for name, got, rest, truth in zip(("gmu", "gsigma"), (gmu, gs), formula(np.float32), formula(np.float64)):
        b = Bound(cid, name)
        b.add(torch.from_numpy(got), torch.from_numpy(rest), torch.from_numpy(truth))
        b.check()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [(1 << 24) + 4, 1 << 24], ids=["n2p24+4-over", "n2p24-under"])
@_stops_the_session_on_a_device_fault
def test_adam_across_2_24_parameters(hip, n):
    import ctypes
    g = _gen(n, 5)
    p0 = torch.randn(n, generator=g, device=DEV)
    grads = [torch.randn(n, generator=g, device=DEV) * s for s in (0.3, 3.0)]
    lr, b1, b2, eps, gs = 1e-3, 0.9, 0.999, 1e-8, 0.5

    def run():
        p, m, v = p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        step, ticket = torch.zeros(1, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        starts, pptr = (ctypes.c_int64 * 2)(0, n), (ctypes.c_void_p * 1)(p.data_ptr())
        for gr in grads:
            hip.call("zs_adam_step_f32", pptr, (ctypes.c_void_p * 1)(gr.data_ptr()), starts, 1, m, v, step, ticket, n, lr, b1, b2, eps, gs, None)
        assert step.cpu().tolist() == [len(grads)] and int(ticket.item()) == 0
        return p, m, v

    def formula(dt):          # zs_hip.h, A1
        p, m, v = p0.to(dt), torch.zeros(n, dtype=dt, device=DEV), torch.zeros(n, dtype=dt, device=DEV)
        for t, gr in enumerate(grads, 1):
            gg = gs * gr.to(dt)
            m = m + (1 - b1) * (gg - m)
            v = b2 * v + (1 - b2) * gg * gg
            p = p - lr / (1 - b1 ** t) * m / (torch.sqrt(v) / math.sqrt(1 - b2 ** t) + eps)
        return p, m, v
    got, again = run(), run()
    cid = "adam-n%d" % n
    for name, a, a2, rest, truth in zip(("param", "exp_avg", "exp_avg_sq"), got, again, formula(F32), formula(F64)):
        assert _bits_equal(a, a2), (cid, name, "second run")
        b = Bound(cid, name)
        b.add(a, rest, truth)
        b.check()


# ---------------------------------------------------------------------------------------------------------------------
# the remaining capped launches of libzs_hip.so (README_variants.md, "Grid caps"): one shape over the cap of grid_for, where the
# grid-stride loop takes a second trip, and its neighbour at the cap
# ---------------------------------------------------------------------------------------------------------------------
def _normal_bwd(x, mu, s, g):            # zs_hip.h, backward of K2
    diff, prec = x - mu, 1 / (s * s)
    t = g * prec * diff
    return -t, t, g * (prec * diff * diff - 1) / s


def _logistic_bwd(x, mu, s, g):          # zs_hip.h, backward of L2
    t = (x - mu) / s
    h = torch.tanh(t / 2)
    return -g * h / s, g * h / s, g * (h * t - 1) / s


BWD_CAPS = [  # entry point, formula, K-summed, (K, R, D) over / under, what is capped
    ("zs_normal_logprob_bwd_f32", _normal_bwd, False, (50, 6991, 3), (50, 6990, 3)),                 # N > 256 * 4096 elements
    ("zs_logistic_logprob_bwd_f32", _logistic_bwd, False, (50, 27963, 3), (50, 27962, 3)),           # N / 4 > 256 * 4096 (k_elem)
    ("zs_normal_logprob_bwd_ksum_f32", _normal_bwd, True, (4, 349526, 3), (4, 349525, 3)),           # M > 256 * 4096 (serial form)
    ("zs_logistic_logprob_bwd_ksum_f32", _logistic_bwd, True, (4, 349526, 3), (4, 349525, 3)),
]


def test_backward_cap_shapes_against_the_caps():
    cap = 256 * GRID_CAP
    for name, _, ksum, (K, R, D), (K2, R2, D2) in BWD_CAPS:
        per = 4 if name == "zs_logistic_logprob_bwd_f32" else 1
        work = (lambda K, R, D: R * D) if ksum else (lambda K, R, D: (K * R * D + per - 1) // per)
        assert work(K, R, D) > cap >= work(K2, R2, D2) and (K, D, R - 1) == (K2, D2, R2)
    assert (4194308 + 3) // 4 > cap >= 4194304 // 4                                # the flat draws below
    assert 262146 * 8 // 4 > 128 * GRID_CAP >= 262144 * 8 // 4 and 349526 * 3 > cap >= 349525 * 3   # observation gradient
    assert 16385 > 4 * GRID_CAP >= 16384 and 4097 > GRID_CAP >= 4096 and (131073 + 7) // 8 > 4 * GRID_CAP >= 131072 // 8


@pytest.mark.gpu
@pytest.mark.parametrize("side", [0, 1], ids=["over", "under"])
@pytest.mark.parametrize("entry", BWD_CAPS, ids=[e[0] for e in BWD_CAPS])
@_stops_the_session_on_a_device_fault
def test_given_value_backward_beyond_the_grid_caps(hip, entry, side):
    name, formula, ksum = entry[:3]
    K, R, D = entry[3 + side]
    M, N = R * D, K * R * D
    g = _gen(K, R, D, 6)
    mu, s = torch.randn(M, generator=g, device=DEV), torch.exp(torch.rand(M, generator=g, device=DEV) * 2 - 1)
    x = (mu + s * 1.5 * torch.randn(K, M, generator=g, device=DEV)).view(-1)
    glp = torch.randn(K, R, generator=g, device=DEV)

    def run():
        outs = [hip.empty(N), hip.empty(M if ksum else N), hip.empty(M if ksum else N)]
        tail = (0,) if "normal" in name else ()
        if ksum:
            hip.call(name, x, mu, s, glp, R, 1, outs[0], outs[1], outs[2], K, R, D, *tail)
        else:
            hip.call(name, x, N, mu, M, s, M, glp, R, 1, outs[0], outs[1], outs[2], K, R, D, *tail)
        return outs

    def evaluate(dt):
        parts = formula(x.to(dt).view(K, R, D), mu.to(dt).view(R, D), s.to(dt).view(R, D), glp.to(dt).view(K, R, 1))
        return [parts[0].reshape(-1)] + [(q.sum(0) if ksum else q).reshape(-1) for q in parts[1:]]
    got, again = run(), run()
    for nm, a, a2, rest, truth in zip(("gx", "gloc", "gscale"), got, again, evaluate(F32), evaluate(F64)):
        assert _bits_equal(a, a2), (name, nm, "second launch")
        b = Bound("%s-K%d-R%d-D%d" % (name, K, R, D), nm)
        b.add(a, rest, truth)
        b.check()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [4194308, 4194304], ids=["over", "under"])
@_stops_the_session_on_a_device_fault
def test_flat_draws_beyond_the_grid_cap(hip, N):
    """k_bern_sample and the element-wise Uniform sampler with u handed in (k_elem): N / 4 groups against 256 * 4096."""
    g = _gen(N, 7)
    p = torch.rand(N, generator=g, device=DEV)
    u, out = hip.empty(N), hip.empty(N)
    hip.call("zs_philox_uniform_f32", u, N, SEED, CALL, None)
    hip.call("zs_bernoulli_sample_f32", p, N, out, N, SEED, CALL, None)
    assert _bits_equal(out, (u < p).float())                                     # bernoulli.py:80
    low, width = torch.randn(4, generator=g, device=DEV), torch.rand(4, generator=g, device=DEV) + 0.5
    high = low + width
    o2, cache = hip.empty(N), hip.empty(N)
    hip.call("zs_uniform_sample_f32", low, 4, high, 4, u, 0, 0, None, o2, cache, N, 1)
    prod = u.view(-1, 4) * (high - low)
    assert _bits_equal(cache, u) and _bits_equal(o2.view(-1, 4), low + prod)     # uniform.py:66-70, two roundings


@pytest.mark.gpu
@pytest.mark.parametrize("K,R,D", [(2, 262146, 8), (2, 262144, 8), (2, 349526, 3), (2, 349525, 3)],
                         ids=["pieces-over", "pieces-under", "scalar-over", "scalar-under"])
@pytest.mark.parametrize("logits", [0, 1])
@_stops_the_session_on_a_device_fault
def test_observation_gradient_beyond_the_grid_caps(hip, K, R, D, logits):
    """zs_bernoulli_logprob_bwd_x with an observation of one plane (Px = R D): the 16-byte form (a wave per 64 pieces, two waves per
    workgroup) and the scalar form (a thread per element)."""
    Px = R * D
    g = _gen(K, R, D, 8)
    p = torch.rand(K, R, D, generator=g, device=DEV) * 0.98 + 0.01
    if logits:
        p = torch.log(p) - torch.log1p(-p)
    glp, scale = torch.randn(R, K, generator=g, device=DEV), torch.rand(R, generator=g, device=DEV) + 0.5

    def run():
        gx = hip.empty(Px)
        hip.call("zs_bernoulli_logprob_bwd_x_f32", p, logits, Px, glp, 1, K, scale, 1, gx, K, R, D)
        return gx

    def evaluate(dt):
        q = _bern_p(p.to(dt), logits)
        rowg = glp.t().to(dt) * scale.to(dt).view(1, R)
        return (rowg.unsqueeze(-1) * (torch.log(q + BERN_EPS) - torch.log((1 - q) + BERN_EPS))).sum(0).reshape(-1)
    got, again = run(), run()
    assert _bits_equal(got, again)
    b = Bound("bwd_x-logits%d-K%d-R%d-D%d" % (logits, K, R, D), "gx")
    b.add(got, evaluate(F32), evaluate(F64))
    b.check()


@pytest.mark.gpu
@pytest.mark.parametrize("B,K", [(16385, 50), (16384, 50), (4097, 70), (4096, 70)], ids=["wave-over", "wave-under", "block-over", "block-under"])
@_stops_the_session_on_a_device_fault
def test_log_mean_exp_beyond_the_grid_caps(hip, B, K):
    x = torch.randn(B, K, generator=_gen(B, K, 9), device=DEV) * 5
    out, again = hip.empty(B), hip.empty(B)
    hip.call("zs_log_mean_exp_f32", x, K, B, K, out)
    hip.call("zs_log_mean_exp_f32", x, K, B, K, again)
    assert _bits_equal(out, again)
    b = Bound("lme-B%d-K%d" % (B, K), "out")
    b.add(out, torch.logsumexp(x, 1) - math.log(K), torch.logsumexp(x.double(), 1) - math.log(K))      # utils.py:6-21
    b.check()


@pytest.mark.gpu
@pytest.mark.parametrize("B,K", [(131073, 20), (131072, 20), (4097, 70), (4096, 70)], ids=["group-over", "group-under", "block-over", "block-under"])
@_stops_the_session_on_a_device_fault
def test_iw_reduce_beyond_the_grid_caps(hip, orc, B, K):
    """k_iw_reduce_group on 8 lanes per datapoint (4096 workgroups x 4 waves x 8 datapoints) and k_iw_reduce_block (K > 64: a
    workgroup per datapoint) against the C oracle, by test_cabi.py's own check."""
    from test_cabi import _check_iw_reduce
    for spread in (1.0, 30.0):
        _check_iw_reduce(hip, orc, B, K, spread)


@pytest.mark.gpu
def test_zz_report_shares_and_peak_memory():
    """Runs last in this file: the share of the factor 16 each case used and the file's peak device memory (README_variants.md)."""
    for k in sorted(SHARES):
        print("share %-70s %.2f of 16" % (k, SHARES[k]))
    if SHARES:
        worst = max(SHARES, key=SHARES.get)
        print("largest share: %.2f (%s)" % (SHARES[worst], worst))
        assert SHARES[worst] <= 16.0
    _CACHE.clear()
    torch.cuda.empty_cache()
    print("peak device memory allocated in this process: %.2f GB" % (torch.cuda.max_memory_allocated() / 1e9))
