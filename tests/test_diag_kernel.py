"""The chain-diagnostics kernels through the raw C ABI of libzs_diag.so (include/zs_diag.h), on the GPU.  See tests/README_diag.md.

Truth: tests/diag_host.py ``reference_*`` -- the header's steps in float64 -- on the recipe's float32 draws widened (the float64
runs take the same values, so one truth serves both dtypes).  Every case runs as a [T, C, E] stack and as a [C, T, E] stack, each
aligned and shifted by one element: all four must agree bit for bit in every output, guard elements around every operand must
survive, the same call again must give the same bits, each output alone (the others NULL) must equal the same output among the
others -- ``rhat`` alone is the R-hat-only mode -- and ``lags`` / ``capped`` must equal the truth exactly.  That last demand is
meaningful because the truth of every case keeps every pair sum P_k it examined at least MIN_P = 1e-9 away from zero (asserted
for every case, none left out): the stop decision is never within rounding of zero.

Bounds of the floating outputs (derived in tests/README_diag.md, not tuned; u = 2^-24 for _f32, 2^-53 for _f64: the one final
rounding; v = 2^-53: the double accumulation; N, M after the split; RATIO = 4 is the file's one constant):
  mean       u |mean| + N M v mean|x|
  var_plus   var_plus (RATIO u + RATIO N M v kappa)          kappa = max_m sum_t (x - mean_m)^2 / (N W)
  rhat       rhat     (RATIO u + RATIO N M v kappa)
  ess        ess      (RATIO u + (lags + 2) RATIO N M v gamma0 / (tau var_plus))          gamma0 = mean_m sum_t d_t^2 / N, which
             bounds mean_m sum_t |d_t d_{t+l}| / N at every lag; tau >= 1 / log10(M N) bounds the division
  acf        RATIO u |acf| + RATIO (T + 2) v
The float32-input torch restatement of tests/diag_host.py is held to the same bounds for every case on the CPU (not gpu)."""
import functools

import numpy as np
import pytest
import torch

import diag_host
from kernel_abi import EINVAL, ENOTSUP, F32, F64, Arena, load, ptr, same_bits, sfx, stream, unit

gpu = pytest.mark.gpu

TS = [4, 5, 8, 9, 64, 65, 257]
CS = [1, 2, 3]
ES = [1, 3, 63, 64, 65, 257, 1025]
SPLITS = [0, 1]
MAX_LAGS = [-1, 1, 6]
RATIO = 4.0
V = 2.0 ** -53
I32 = torch.int32
FLOATS = ("mean", "var_plus", "rhat", "ess")
WORST = {}          # quantity -> the worst error / bound seen in this session (printed; recorded in README_diag.md)


def cases_of(T):
    """(C, E, split, max_lag) for this T: every C x E, split and max_lag cycling so that the six combinations come round."""
    out, i = [], TS.index(T)
    for C in CS:
        for E in ES:
            out.append((C, E, SPLITS[i % 2], MAX_LAGS[i % 3]))
            i += 1
    return out


@functools.lru_cache(maxsize=None)
def truth(T, C, E, split, max_lag, case=0):
    """(the recipe's draws [T, C, E] float32 numpy, the float64 truth); asserts the margin of the stop decision."""
    x = diag_host.recipe(T, C, E, case)
    r = diag_host.reference_summary(torch.from_numpy(x), split, max_lag)
    assert float(r["min_abs_p"].min()) >= diag_host.MIN_P, "T=%d C=%d E=%d: a pair sum within %g of zero; change `case`" % (T, C, E, diag_host.MIN_P)
    return x, r


def bounds(dtype, r):
    u, NM = unit(dtype), r["N"] * r["M"]
    rel = RATIO * u + RATIO * NM * V * r["kappa"]
    rel_ess = RATIO * u + (r["lags"].to(F64) + 2) * RATIO * NM * V * r["gamma0"] / (r["tau"] * r["var_plus"])
    return dict(mean=u * r["mean"].abs() + NM * V * r["absx"], var_plus=rel * r["var_plus"], rhat=rel * r["rhat"], ess=rel_ess * r["ess"])


def assert_close(name, got, want, tol):
    got = got.detach().cpu().to(F64).reshape(want.shape)
    assert not bool(torch.isnan(got).any()), "%s: NaN" % name
    err = (got - want).abs()
    ratio = float((err / tol.clamp(min=1e-320)).max()) if err.numel() else 0.0
    key = name.split(" [")[0]
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print("%s: worst error / bound = %.3f" % (name, ratio))
    assert bool((err <= tol).all()), "%s: %d elements out of bounds, worst error / bound %.3f" % (name, int((err > tol).sum()), ratio)


def check_case(tag, dtype, r, res):
    b = bounds(dtype, r)
    assert torch.equal(res["lags"].cpu(), r["lags"]), "lags differ from the truth" + tag
    assert torch.equal(res["capped"].cpu(), r["capped"]), "capped differs from the truth" + tag
    for name in FLOATS:
        assert_close(name + tag, res[name], r[name], b[name])


def print_worst():
    print("worst error / bound so far: %s" % ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


# ------------------------------------------------------------------------------------------------ the CPU cross-check (not gpu)
@pytest.mark.parametrize("T", TS)
def test_float32_restatement_stays_inside_the_bounds(T):
    for C, E, split, max_lag in cases_of(T):
        x, r = truth(T, C, E, split, max_lag)
        tce = torch.from_numpy(x)
        cte = tce.permute(1, 0, 2).contiguous()
        a = dict(zip(diag_host.OUTPUTS, diag_host.summary(tce, C * E, E, T, C, E, split, max_lag)))
        b = dict(zip(diag_host.OUTPUTS, diag_host.summary(cte, E, T * E, T, C, E, split, max_lag)))
        for name in diag_host.OUTPUTS:
            assert same_bits(a[name], b[name]), name
        check_case(" [torch: T=%d C=%d E=%d split %d max_lag %d]" % (T, C, E, split, max_lag), F32, r, a)
    print_worst()


def test_the_issue_shapes_keep_the_margin_split_and_unsplit():
    for T, C, E in ((8, 1, 3), (9, 2, 5), (64, 4, 7), (65, 4, 130), (257, 3, 65), (1000, 2, 4)):
        for split in SPLITS:
            if (T // 2 if split else T) >= 2:
                truth(T, C, E, split, -1)


# ------------------------------------------------------------------------------------------------ device plumbing
@pytest.fixture(scope="module")
def lib():
    return load("diag")


def place(ar, x, dtype, layout):
    """(device view, st, sc) of the draws x [T, C, E] stored as 'tce' or 'cte'"""
    T, C, E = x.shape
    if layout == "tce":
        return ar.put(x, dtype), C * E, E
    return ar.put(np.ascontiguousarray(x.transpose(1, 0, 2)), dtype), E, T * E


def run_summary(lib, dtype, x, split, max_lag, layout="tce", shift=0, want=diag_host.OUTPUTS, repeat=False):
    """One zs_diag_summary call (twice with ``repeat``: the same bits); dict of the wanted outputs."""
    T, C, E = x.shape
    ar = Arena(shift)
    xd, st, sc = place(ar, x, dtype, layout)
    res = None
    for rep in range(2 if repeat else 1):
        outs = {n: ar.out(E, I32 if n in ("lags", "capped") else dtype) for n in want}
        rc = lib.raw("zs_diag_summary" + sfx(dtype), ptr(xd), st, sc, T, C, E, split, max_lag,
                     *([ptr(outs.get(n)) for n in diag_host.OUTPUTS] + [stream()]))
        assert rc == 0, rc
        torch.cuda.synchronize()
        out = {n: t.cpu() for n, t in outs.items()}
        if res is None:
            res = out
        else:
            for n in res:
                assert same_bits(res[n], out[n]), "two identical calls differ in %s" % n
    ar.check_guards()
    return res


@gpu
@pytest.mark.parametrize("T", TS)
def test_summary_against_float64(lib, T):
    for C, E, split, max_lag in cases_of(T):
        x, r = truth(T, C, E, split, max_lag)
        for dtype in (F32, F64):
            ref = run_summary(lib, dtype, x, split, max_lag, repeat=True)
            for layout, shift in (("tce", 1), ("cte", 0), ("cte", 1)):
                other = run_summary(lib, dtype, x, split, max_lag, layout, shift)
                for n in ref:
                    assert same_bits(ref[n], other[n]), "%s differs in layout %s shift %d (T=%d C=%d E=%d)" % (n, layout, shift, T, C, E)
            for n in diag_host.OUTPUTS:          # each output alone; `rhat` alone is the R-hat-only mode
                alone = run_summary(lib, dtype, x, split, max_lag, want=(n,))
                assert same_bits(alone[n], ref[n]), "%s alone differs from %s among the others (T=%d C=%d E=%d)" % (n, n, T, C, E)
            check_case(" [T=%d C=%d E=%d split %d max_lag %d %s]" % (T, C, E, split, max_lag, sfx(dtype)), dtype, r, ref)
    print_worst()


@gpu
def test_a_wide_case_crosses_many_workgroups(lib):
    T, C, E = 16, 2, 2 ** 16 + 5
    x, r = truth(T, C, E, 1, -1)
    for dtype in (F32, F64):
        ref = run_summary(lib, dtype, x, 1, -1, repeat=True)
        other = run_summary(lib, dtype, x, 1, -1, "cte", 1)
        for n in ref:
            assert same_bits(ref[n], other[n]), n
        check_case(" [wide %s]" % sfx(dtype), dtype, r, ref)
    print_worst()


@gpu
@pytest.mark.parametrize("T,C,split", [(12, 9, 1), (12, 17, 0), (9, 16, 0)])
def test_more_chains_than_a_lane_keeps_means_of(lib, T, C, split):
    """A lane keeps 16 chain means and sums those of further chains again (zs_diag_math.h): M = 18 and 17 take that path, 16 not."""
    E = 65
    x, r = truth(T, C, E, split, -1)
    for dtype in (F32, F64):
        ref = run_summary(lib, dtype, x, split, -1, repeat=True)
        other = run_summary(lib, dtype, x, split, -1, "cte", 1)
        for n in ref:
            assert same_bits(ref[n], other[n]), n
        check_case(" [T=%d C=%d split %d %s]" % (T, C, split, sfx(dtype)), dtype, r, ref)


@gpu
def test_a_nan_draw_and_a_constant_series_leave_their_neighbours_alone(lib):
    T, C, E = 64, 2, 65
    x, _ = truth(T, C, E, 1, -1)
    bad = x.copy()
    bad[7, 1, 5] = np.nan
    bad[3, 0, 9] = np.inf
    bad[:, :, 40] = 1.5
    hit = [5, 9, 40]
    others = [e for e in range(E) if e not in hit]
    for dtype in (F32, F64):
        for split in SPLITS:
            good, res = run_summary(lib, dtype, x, split, -1), run_summary(lib, dtype, bad, split, -1)
            for n in diag_host.OUTPUTS:
                assert same_bits(good[n][others], res[n][others]), "a neighbour changed in %s" % n
            for e in (5, 9):
                assert all(bool(torch.isnan(res[n][e])) for n in FLOATS), "a non-finite draw must give NaN"
            assert float(res["mean"][40]) == 1.5 and float(res["var_plus"][40]) == 0.0
            assert bool(torch.isnan(res["rhat"][40])) and bool(torch.isnan(res["ess"][40])), "a constant series has no ratio"
            assert res["lags"][hit].tolist() == [0, 0, 0] and res["capped"][hit].tolist() == [0, 0, 0]


@gpu
@pytest.mark.parametrize("T", [TS[0], TS[-1]])
def test_autocorr_against_float64(lib, T):
    for C in CS:
        for E in (1, 65, 1025):
            x = diag_host.recipe(T, C, E)
            xt = torch.from_numpy(x)
            for L in (0, 1, T - 1):
                want = diag_host.reference_autocorr(xt, L)
                for dtype in (F32, F64):
                    runs = []
                    for layout, shift in (("tce", 0), ("tce", 0), ("tce", 1), ("cte", 0), ("cte", 1)):
                        ar = Arena(shift)
                        xd, st, sc = place(ar, x, dtype, layout)
                        acf = ar.out((L + 1) * C * E, dtype)
                        assert lib.raw("zs_diag_autocorr" + sfx(dtype), ptr(xd), st, sc, T, C, E, L, ptr(acf), stream()) == 0
                        ar.check_guards()
                        runs.append(acf.cpu().view(L + 1, C, E))
                    for other in runs[1:]:
                        assert same_bits(runs[0], other), "acf differs between layouts, alignments or calls"
                    assert bool((runs[0][0] == 1).all())
                    assert_close("acf [T=%d C=%d E=%d L=%d %s]" % (T, C, E, L, sfx(dtype)), runs[0], want,
                                 RATIO * unit(dtype) * want.abs() + RATIO * (T + 2) * V)
    print_worst()


@gpu
def test_rejected_arguments_write_nothing(lib):
    T, C, E = 8, 2, 5
    x = diag_host.recipe(T, C, E)
    big = 2 ** 31
    for dtype in (F32, F64):
        ar = Arena(0)
        xd = ar.put(x, dtype)
        o = [ar.out(E, dtype) for _ in range(4)] + [ar.out(E, I32), ar.out(E, I32)]
        acf = ar.out(T * C * E, dtype)
        po, st = [ptr(t) for t in o], stream()

        def summ(x_=xd, st_=C * E, sc_=E, T_=T, C_=C, E_=E, split=1, outs=po):
            return lib.raw("zs_diag_summary" + sfx(dtype), ptr(x_), st_, sc_, T_, C_, E_, split, -1, *(outs + [st]))

        def auto(x_=xd, st_=C * E, sc_=E, T_=T, C_=C, E_=E, L=1, acf_=acf):
            return lib.raw("zs_diag_autocorr" + sfx(dtype), ptr(x_), st_, sc_, T_, C_, E_, L, ptr(acf_), st)
        for f in (summ, auto):
            assert f(x_=None) == EINVAL
            assert f(T_=-1) == EINVAL and f(C_=-1) == EINVAL and f(E_=-1) == EINVAL
            assert f(E_=big) == ENOTSUP
            assert f(T_=0) == 0 and f(C_=0) == 0 and f(E_=0) == 0          # T C E == 0 launches nothing
            assert f(sc_=E - 1) == EINVAL and f(st_=C * E - 1) == EINVAL          # a stride below the extent it steps over
            assert f(st_=E, sc_=T * E - 1) == EINVAL and f(st_=E - 1, sc_=T * E) == EINVAL
            assert f(st_=-C * E) == EINVAL
        assert summ(outs=[None] * 6) == EINVAL and auto(acf_=None) == EINVAL          # nothing to write
        assert summ(T_=3) == EINVAL and summ(T_=1, split=0) == EINVAL                    # N < 2 after the split
        assert auto(L=T) == EINVAL and auto(L=-1) == EINVAL
        torch.cuda.synchronize()
        assert ar.untouched(), "a rejected call wrote something"
        assert summ(T_=2, split=0) == 0 and summ(C_=1, sc_=0) == 0          # N = 2 runs; with one chain sc is not looked at
        ar.check_guards()
    assert lib.cdll.zs_diag_abi_version() == 1
