"""The matrix-variate-normal kernels through the raw C ABI of libzs_matvar.so (include/zs_matvar.h), on the GPU.  See
tests/README_matvar.md.

Truth: the header's formulas in float64 torch on the CPU (``truth`` below), on float32-representable inputs, so one truth serves
_f32 and _f64.  The upper triangles of the factors handed to a kernel are NaN: they are never read.  Every case runs with aligned
operands and with every operand shifted by one element: the two must agree bit for bit, the guards around every operand and
workspace must survive, and the same calls twice must give the same bits.

Tolerances (derived, not tuned; the worst error / bound the MI355X gave is recorded in README_matvar.md; u = 2^-24 for _f32, 2^-53
for _f64; RATIO = 4; Higham, Accuracy and Stability, ch. 8, for the substitutions).  |.| is elementwise, products of |.| are matrix
products.  A solve with a dim x dim factor L is blocked: off-diagonal updates of at most dim terms, then a product with the
explicitly inverted 16 x 16 diagonal block, itself the result of a 16-step substitution -- c_dim = dim + 20 roundings in all.  The
explicit inverse costs a second conditioning factor: with M_L = |L^-1| |L| the computed W of L W = C has
  |dW| <= c_dim u (M_L + M_L^2) |W| + |L^-1| |dC|                    (M_L of L^T for the transposed solves)
  Y = U^-1 (X - mean):  e_Y = |U^-1| u (|X| + |mean|) + c_n u (M_U + M_U^2) |Y|
  A = Y V^-T:           e_A = e_Y |V^-T| + c_p u |A| (M_V + M_V^2)^T          and likewise e_B (B = U^-T A), e_C (C = A V^-1), e_S
  sums: the n16 p16 elements of |E|^2 / |A|^2 go 256 threads wide, then a butterfly and four waves: s = ceil(n16 p16 / 256) + 16
  M1 z    (n + p + 3) u (|mean| + |U| |E| |V|^T);    M1 lp  s u (sum of the magnitudes of its terms);   M2 lp  that + sum |A| e_A
  gX      |g| e_S + u |g S|;     gmean  sum_k |g| e_S + (2 K + 3) u sum_k |g S|      (a k-sum: at most K terms and K shares)
  gU      sum_k |g| (e_B |A|^T + |B| e_A^T) + (p + 2 K + 8) u (sum_k |g| |B| |A|^T + diag(p sum_k |g| / U_ii));  gV alike with n, C^T A
  M1 bwd  gmean (2 K + 3) u sum_k |gZ|;  gU (2 p + 2 K + 8) u (sum_k |gZ| |V| |E|^T + diag);  gV (2 n + 2 K + 8) u (sum_k |gZ|^T |U| |E| + diag)"""
import functools
import math

import numpy as np
import pytest
import torch

from kernel_abi import DEV, EINVAL, ENOTSUP, F32, F64, I64, Arena, load, load_main, ptr, same_bits, sfx, stream, unit

pytestmark = pytest.mark.gpu

RATIO = 4
RK = [(1, 1), (1, 5), (3, 2)]
# one ragged block, exactly one block, one block plus a row, an update over more than one earlier block, different block counts on
# the two axes, the caps; (R, K) cycles so that every shape class meets a k-sum of several particles and more than one row
SHAPES = [(1, 1), (16, 16), (17, 15), (33, 3), (3, 33), (64, 64), (15, 64), (1, 17), (64, 16), (33, 33)]
WIDE = [(65, 17), (17, 128), (128, 128)]          # above the float64 cap: _f32 only
# K = 19 over one row is cut into 10 shares of 2 particles, the last of 1: a workgroup walks more than one particle (its partials
# added to, the tiles staged again over the previous particle's), and the last share is ragged; K <= 5 gives one particle a share
WALKED = [(17, 15, 1, 19), (33, 3, 1, 19)]
CASES = [(n, p) + RK[i % 3] + ((F32, F64),) for i, (n, p) in enumerate(SHAPES)] + \
        [(n, p) + RK[(i + 1) % 3] + ((F32,),) for i, (n, p) in enumerate(WIDE)] + [c + ((F32, F64),) for c in WALKED]
WORST = {}          # quantity -> the worst error / tolerance seen in this session (printed; recorded in README_matvar.md)


def f32r(a):
    return torch.from_numpy(np.asarray(a).astype(np.float32).astype(np.float64))


def factor(rng, R, d):
    L = np.tril(rng.standard_normal((R, d, d)) * 0.5 / math.sqrt(d), -1)
    L[:, np.arange(d), np.arange(d)] = rng.uniform(0.5, 2.0, (R, d))
    L[:, np.triu_indices(d, 1)[0], np.triu_indices(d, 1)[1]] = np.nan
    return f32r(L)


def case_inputs(n, p, R, K):
    rng = np.random.default_rng(100000 * n + 100 * p + 10 * R + K)
    mean = f32r(3.0 * rng.standard_normal((R, n, p)))
    return dict(U=factor(rng, R, n), V=factor(rng, R, p), mean=mean, x=f32r(mean.numpy()[None] + 2.0 * rng.standard_normal((K, R, n, p))),
                eps=f32r(rng.standard_normal((K, R, n, p))), g=f32r(rng.standard_normal((K, R))), gz=f32r(rng.standard_normal((K, R, n, p))))


def low(L):
    return torch.tril(torch.nan_to_num(L, nan=0.0))


def solve(L, C, trans=False):
    """L^-1 C, or L^-T C"""
    return torch.linalg.solve_triangular(L.mT if trans else L, C, upper=trans)


def truth(d, x=None):
    """every quantity of the header in float64; ``x`` replaces the case's value"""
    U, V, mean, eps, g, gz = low(d["U"]), low(d["V"]), d["mean"], d["eps"], d["g"], d["gz"]
    x = d["x"] if x is None else x
    n, p = mean.shape[-2:]
    t = dict(U=U, V=V)
    c = -0.5 * n * p * math.log(2 * math.pi) - p * torch.log(torch.diagonal(U, dim1=-2, dim2=-1)).sum(-1) - n * torch.log(torch.diagonal(V, dim1=-2, dim2=-1)).sum(-1)
    du = torch.diag_embed(p * g.sum(0)[:, None] / torch.diagonal(U, dim1=-2, dim2=-1))
    dv = torch.diag_embed(n * g.sum(0)[:, None] / torch.diagonal(V, dim1=-2, dim2=-1))
    t["z"], t["lp1"] = mean + U @ eps @ V.mT, c - 0.5 * (eps ** 2).sum((-1, -2))
    t["gm1"], t["gu1"], t["gv1"] = gz.sum(0), torch.tril((gz @ V @ eps.mT).sum(0)) - du, torch.tril((gz.mT @ U @ eps).sum(0)) - dv
    Y = solve(U, x - mean)
    A = solve(V, Y.mT).mT
    B, C = solve(U, A, True), solve(V, A.mT, True).mT
    S = solve(V, B.mT, True).mT
    w = g[..., None, None]
    t.update(Y=Y, A=A, B=B, C=C, S=S, lp2=c - 0.5 * (A ** 2).sum((-1, -2)), gx=-w * S, gm2=(w * S).sum(0),
             gu2=torch.tril((w * B @ A.mT).sum(0)) - du, gv2=torch.tril((w * C.mT @ A).sum(0)) - dv)
    t["const"] = 0.5 * n * p * math.log(2 * math.pi) + p * torch.log(torch.diagonal(U, dim1=-2, dim2=-1)).abs().sum(-1) + n * torch.log(torch.diagonal(V, dim1=-2, dim2=-1)).abs().sum(-1)
    return t


def bounds(dtype, d, t, K, x=None):
    """the tolerances of the module docstring, same keys as ``truth``"""
    u, mean, eps, gz = unit(dtype), d["mean"], d["eps"], d["gz"]
    x = d["x"] if x is None else x
    n, p = mean.shape[-2:]
    U, V, ga = t["U"], t["V"], d["g"].abs()[..., None, None]
    aU, aV, iU, iV = U.abs(), V.abs(), torch.linalg.inv(U).abs(), torch.linalg.inv(V).abs()
    cn, cp = n + 20, p + 20
    s = math.ceil(16 * math.ceil(n / 16) * 16 * math.ceil(p / 16) / 256) + 16

    def amp(iL, aL, trans):
        M = (iL.mT @ aL.mT) if trans else (iL @ aL)
        return M + M @ M

    Y, A, B, C, S = (t[k].abs() for k in "YABCS")
    eY = iU @ (u * (x.abs() + mean.abs())) + cn * u * amp(iU, aU, False) @ Y
    eA = eY @ iV.mT + cp * u * A @ amp(iV, aV, False).mT
    eB = iU.mT @ eA + cn * u * amp(iU, aU, True) @ B
    eC = eA @ iV + cp * u * C @ amp(iV, aV, True).mT
    eS = eB @ iV + cp * u * S @ amp(iV, aV, True).mT
    du = torch.diag_embed(p * ga[..., 0, 0].sum(0)[:, None] / torch.diagonal(U, dim1=-2, dim2=-1))
    dv = torch.diag_embed(n * ga[..., 0, 0].sum(0)[:, None] / torch.diagonal(V, dim1=-2, dim2=-1))
    b = dict(z=(n + p + 3) * u * (mean.abs() + aU @ eps.abs() @ aV.mT), lp1=s * u * (0.5 * (eps ** 2).sum((-1, -2)) + t["const"]),
             lp2=s * u * (0.5 * (A ** 2).sum((-1, -2)) + t["const"]) + (A * eA).sum((-1, -2)),
             gx=ga * eS + u * ga * S, gm2=(ga * eS).sum(0) + (2 * K + 3) * u * (ga * S).sum(0),
             gu2=(ga * (eB @ A.mT + B @ eA.mT)).sum(0) + (p + 2 * K + 8) * u * ((ga * B @ A.mT).sum(0) + du),
             gv2=(ga * (eC.mT @ A + C.mT @ eA)).sum(0) + (n + 2 * K + 8) * u * ((ga * C.mT @ A).sum(0) + dv),
             gm1=(2 * K + 3) * u * gz.abs().sum(0), gu1=(2 * p + 2 * K + 8) * u * ((gz.abs() @ aV @ eps.abs().mT).sum(0) + du),
             gv1=(2 * n + 2 * K + 8) * u * ((gz.abs().mT @ aU @ eps.abs()).sum(0) + dv))
    return {k: RATIO * v + 1e-300 for k, v in b.items()}


@pytest.fixture(scope="module")
def lib():
    return load("matvar")


@pytest.fixture(scope="module")
def main_lib():
    return load_main()


def part_of(lib, ar, dtype, which, K, R, n, p):
    """the guarded `part` workspace (one element where the arguments are rejected)"""
    return ar.out(max(lib.raw("zs_matvar_workspace_elems", which, 4 if dtype == F32 else 8, K, R, n, p), 1), dtype)


def m1(lib, dtype, ar, o, K, R, n, p, eps, seed=0, call=0, rs=None):
    """(return codes, z, lp, gmean, gu, gv) of M1 and its backward; o = device operands by name"""
    s = sfx(dtype)
    z, lp, gm, gu, gv = (ar.out(c, dtype) for c in (K * R * n * p, K * R, R * n * p, R * n * n, R * p * p))
    part = part_of(lib, ar, dtype, 0, K, R, n, p)
    rcs = [lib.raw("zs_matvar_sample_logprob" + s, ptr(o["mean"]), ptr(o["U"]), ptr(o["V"]), ptr(eps), ptr(z), ptr(lp), K, R, n, p, seed,
                   call, ptr(rs), stream()),
           lib.raw("zs_matvar_sample_logprob_bwd" + s, ptr(o["U"]), ptr(o["V"]), ptr(eps), ptr(o["gz"]), ptr(o["g"]), ptr(part), ptr(gm),
                   ptr(gu), ptr(gv), K, R, n, p, seed, call, ptr(rs), stream())]
    return rcs, z, lp, gm, gu, gv


def m2(lib, dtype, ar, o, K, R, n, p, x, px=None):
    """(return codes, lp, gx, gmean, gu, gv) of M2 and its backward at the value x"""
    s = sfx(dtype)
    px = x.numel() if px is None else px
    lp, gx, gm, gu, gv = (ar.out(c, dtype) for c in (K * R, K * R * n * p, R * n * p, R * n * n, R * p * p))
    part = part_of(lib, ar, dtype, 1, K, R, n, p)
    rcs = [lib.raw("zs_matvar_logprob" + s, ptr(o["mean"]), ptr(o["U"]), ptr(o["V"]), ptr(x), px, ptr(lp), K, R, n, p, stream()),
           lib.raw("zs_matvar_logprob_bwd" + s, ptr(o["mean"]), ptr(o["U"]), ptr(o["V"]), ptr(x), px, ptr(o["g"]), ptr(part), ptr(gx),
                   ptr(gm), ptr(gu), ptr(gv), K, R, n, p, stream())]
    return rcs, lp, gx, gm, gu, gv


def assert_close(name, got, want, tol):
    got = got.cpu().to(F64).view(want.shape)
    err = (got - want).abs()
    ratio = float((err / tol).max())
    WORST[name.split(" [")[0]] = max(WORST.get(name.split(" [")[0], 0.0), ratio)
    print("%s: worst error / tolerance = %.3f" % (name, ratio))
    assert bool(torch.isfinite(got).all()), "%s: non-finite values" % name
    assert bool((err <= tol).all()), "%s: %d elements out of tolerance, worst error / tolerance %.3f" % (name, int((err > tol).sum()), ratio)
    return ratio


def same(a, b, what):
    assert a[0] == [0, 0] and b[0] == [0, 0], what
    for x, y in zip(a[1:], b[1:]):
        assert same_bits(x, y), what


GOT = ("z", "lp1", "gm1", "gu1", "gv1", "lp2", "gx", "gm2", "gu2", "gv2", "lpz")


@functools.lru_cache(maxsize=2)
def case_truth(n, p, R, K):
    """the inputs of a shape and their truth, computed once and left unchanged"""
    d = case_inputs(n, p, R, K)
    return d, truth(d)


def check_case(lib, main_lib, n, p, R, K, dtypes):
    """M1, M2 and both backwards in both layouts, twice, against the truth.  Returns ({dtype: {name of GOT: result of the aligned
    layout, on the CPU}}, {name: worst error / tolerance})."""
    d, t = case_truth(n, p, R, K)
    outs, worst = {}, {}
    count, seed, call = K * R * n * p, 11 + n, 3 + p
    rs = torch.tensor((77, 1 << 33), dtype=I64, device=DEV) if (n + p) % 2 else None          # the launch's stream by value, or by rng_state
    noise = torch.empty(count, dtype=F32, device=DEV)
    main_lib.call("zs_philox_normal_f32", noise.data_ptr(), count, seed, call, ptr(rs), stream())
    for dtype in dtypes:
        res = []
        for shift in (0, 1):
            ar = Arena(shift)
            o = {k: ar.put(v, dtype) for k, v in d.items()}
            one, again = m1(lib, dtype, ar, o, K, R, n, p, o["eps"]), m1(lib, dtype, ar, o, K, R, n, p, o["eps"])
            two, again2 = m2(lib, dtype, ar, o, K, R, n, p, o["x"]), m2(lib, dtype, ar, o, K, R, n, p, o["x"])
            same(one, again, "two identical calls differ")
            same(two, again2, "two identical calls differ")
            at_z = m2(lib, dtype, ar, o, K, R, n, p, one[1])
            shared = ar.put(d["x"][0], dtype)
            same(m2(lib, dtype, ar, o, K, R, n, p, shared), m2(lib, dtype, ar, o, K, R, n, p, ar.put(d["x"][0][None].expand(K, R, n, p).contiguous(), dtype)),
                 "a value without the particle axis differs from its expansion")
            same(m1(lib, dtype, ar, o, K, R, n, p, None, seed, call, rs), m1(lib, dtype, ar, o, K, R, n, p, ar.put(noise.cpu().view(K, R, n, p), dtype)),
                 "the in-kernel draw is not the injected Philox stream")
            ar.check_guards()
            res.append([a.cpu() for a in one[1:] + two[1:] + at_z[1:2]])
        for a, b in zip(*res):
            assert same_bits(a, b), "the aligned and the shifted layout differ"
        got = dict(zip(GOT, res[0]))
        tol = bounds(dtype, d, t, K)
        tag = " [n=%d p=%d R=%d K=%d %s]" % (n, p, R, K, sfx(dtype))
        for k in ("gu1", "gu2", "gv1", "gv2"):
            dim = n if k[1] == "u" else p
            assert bool((torch.triu(got[k].view(R, dim, dim), 1) == 0).all()), "%s: the upper triangle is not exactly zero" % k
        for k in ("z", "lp1", "gm1", "gu1", "gv1", "lp2", "gx", "gm2", "gu2", "gv2"):
            worst[k + sfx(dtype)] = assert_close(k + tag, got[k], t[k], tol[k])
        # M2 at M1's own z against M1's lp: within the sum of the two bounds
        zd = got["z"].to(F64).view(K, R, n, p)
        tz = truth(d, zd)
        assert_close("lp(z)" + tag, got["lpz"], got["lp1"].to(F64).view(K, R), tol["lp1"] + bounds(dtype, d, tz, K, zd)["lp2"])
        outs[dtype] = got
    return outs, worst


@pytest.mark.parametrize("n,p,R,K,dtypes", CASES)
def test_forward_and_backward_against_float64(lib, main_lib, n, p, R, K, dtypes):
    check_case(lib, main_lib, n, p, R, K, dtypes)
    print("worst error / tolerance so far: %s" % ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def test_rejected_arguments_write_nothing(lib):
    n, p, R, K = 5, 4, 3, 2
    d = case_inputs(n, p, R, K)
    for dtype, over in ((F32, 129), (F64, 65)):
        ar = Arena(0)
        o = {k: ar.put(v, dtype) for k, v in d.items()}
        nulled = dict(o, U=None)
        assert m1(lib, dtype, ar, nulled, K, R, n, p, o["eps"])[0] == [EINVAL] * 2 and m2(lib, dtype, ar, nulled, K, R, n, p, o["x"])[0] == [EINVAL] * 2
        assert m1(lib, dtype, ar, o, K, R, 0, p, o["eps"])[0] == [EINVAL] * 2 and m2(lib, dtype, ar, o, K, R, 0, p, o["x"], 1)[0] == [EINVAL] * 2
        assert m2(lib, dtype, ar, o, K, R, n, p, o["x"], K * R * n * p + 1)[0] == [EINVAL] * 2          # a period that is none
        assert m1(lib, dtype, ar, o, K, R, over, p, o["eps"])[0] == [ENOTSUP] * 2 and m2(lib, dtype, ar, o, K, R, n, over, o["x"], 1)[0] == [ENOTSUP] * 2
        torch.cuda.synchronize()
        assert ar.untouched(), "a rejected call wrote something"
    assert [lib.raw("zs_matvar_max_dim", nb) for nb in (4, 8, 2)] == [128, 64, 0]
    assert [lib.raw("zs_matvar_shares", k, r) for k, r in ((5, 1), (50, 1), (5, 64), (2, 1000), (0, 3))] == [5, 13, 3, 1, 0]
    assert lib.raw("zs_matvar_shares", 19, 1) == 10          # what the WALKED cases rely on
