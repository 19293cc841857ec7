"""The admixture-likelihood kernels through the raw C ABI of libzs_topic.so (include/zs_topic.h), on the GPU.  See
tests/README_topic.md.

Truth: the header's formulas in float64 torch on the CPU (``truth`` below), on float32-representable inputs, so one truth serves
_f32 and _f64.  Every case runs with aligned operands and with every operand shifted by one element: the two must agree bit for
bit, the guard elements around every operand and workspace must survive, and the same calls twice must give the same bits.

Inputs.  H = o_r + 3 N(0,1), B = p_k + 2 N(0,1) with offsets cycling through {-80, 0, +80}, one column of B lowered by 90 in every
topic, X ~ Poisson(0.3) with row 0 all zero (where X has more than one row), g ~ N(0,1).  A row of H spreads a few sigma of 3, far
below 60 nats: every case is inside the domain the header states.

Tolerances (derived, not tuned; the worst error / bound the MI355X gave is recorded in README_topic.md; u = 2^-24 for _f32,
2^-53 for _f64; RATIO = 4).  Every product under the logarithm is positive, so there is no cancellation before it.
  E_exp[v] = |H|_max + |B|_max + |lse|_max + |c_v| + 4     the rounding of the exponents' arguments (each a difference of
             numbers of that size) and two device exp / log calls at 2 ulp each: the prologue and the staging call the device
             library's expf / logf / exp / log, for which no header of the project states a bound (the epilogue's logarithm is
             zs_common.h's ln_fast, v_log_f32 at 1 ulp, within the same allowance)
  e[r,v]   = u ((K + 4) + E_exp[v] + |log pred[r,v]|)      log pred: K-term positive dot product, the shifts, the final rounding;
             also bounds the relative error of pred, of phi (u E_exp) and of theta (u (K + 4 + E_exp))
  lp       RATIO [ sum_v x e + (V_nz + panels) u sum_v x |log pred| ]          V_nz non-zero terms, summed in a fixed order
  dtheta   t[r,k] = sum_v |W| phi 2 e + (V_nz + panels + 4) u sum_v |W| phi    W = g x / pred carries e, phi carries <= e
  dH       RATIO theta [ t + u (K + 4 + max E_exp) (sum_v |W| phi + |g| N) ]
  A        a[k,v] = sum_r theta |W| 2 e + (R_nz + 4) u sum_r theta |W|         A = sum_r theta W, R_nz non-zero terms
  s_k      c[k]   = sum_v phi a + (V + panels + 4 + max E_exp) u sum_v phi |A|
  dB       RATIO { phi [ a + c + u (E_exp + 4) (|A| + |s_k|) ] + tiny (|s_k| + 2) }
           tiny = the smallest normal number of the format.  dB = T - phi s_k: T = phi A is formed from the shifted operands, all
           in (0, 1], and keeps its relative bound, but the second term multiplies phi itself, and the lowered column has
           phi ~ 1e-43, below float32's normal range, where a value is held to the subnormal spacing or flushed: an absolute error
           of at most tiny in phi, times |s_k|, and at most tiny in each of the two roundings of the result
`panels` is counted at the narrower panel (32 columns), which is also at least the number of column splits of grad_doc."""
import functools

import numpy as np
import pytest
import torch

from kernel_abi import EINVAL, ENOTSUP, F32, F64, Arena, load, ptr, same_bits, sfx, stream, unit, untouched

pytestmark = pytest.mark.gpu

RATIO = 4
KS = [1, 3, 4, 5, 50, 64, 128]
VS = [1, 15, 17, 64, 65, 1000]
SHAPES = [(1, 1), (1, 17), (3, 5), (2, 33)]
# a cycling subset of the product: every K twice, every V at least twice, every shape at least three times, K = 128 with V = 1000;
# the count matrix is shared (Dx = docs) except in case 2, where it is full (Dx = R)
CASES = [(KS[i % 7], VS[(5 - i) % 6], SHAPES[i % 4], i == 2) for i in range(14)]
WORST = {}          # quantity -> the worst error / tolerance seen in this session (printed; recorded in README_topic.md)


def f32r(a):
    return torch.from_numpy(np.asarray(a).astype(np.float32).astype(np.float64))


def case_inputs(K, V, chains, docs, full):
    rng = np.random.default_rng(100000 * K + 100 * V + 10 * chains + docs)
    R, Dx = chains * docs, (chains * docs if full else docs)
    off = np.array([-80.0, 0.0, 80.0])
    H = f32r(off[np.arange(R) % 3][:, None] + 3.0 * rng.standard_normal((R, K)))
    B = off[np.arange(K) % 3][:, None] + 2.0 * rng.standard_normal((K, V))
    B[:, V // 2] -= 90.0
    X = rng.poisson(0.3, (Dx, V)).astype(np.float64)
    if Dx > 1:
        X[0] = 0.0
    return H, f32r(B), torch.from_numpy(X), f32r(rng.standard_normal(R))


def truth(H, B, X, g):
    """(lp, dH, dB) and what the bounds need, in float64"""
    R = H.shape[0]
    Xr = X[torch.arange(R) % X.shape[0]]
    th, ph = torch.softmax(H, -1), torch.softmax(B, -1)
    pred = th @ ph
    logp = torch.log(pred)
    lp = torch.where(Xr > 0, Xr * logp, torch.zeros_like(logp)).sum(-1)
    W = g[:, None] * Xr / pred
    dth, N = W @ ph.T, Xr.sum(-1)
    A = th.T @ W
    s = (th * dth).sum(0)
    return dict(lp=lp, dH=th * (dth - (g * N)[:, None]), dB=ph * (A - s[:, None]), Xr=Xr, th=th, ph=ph, logp=logp, W=W, N=N, A=A, s=s)


def bounds(dtype, H, B, g, t):
    u, (R, K), V = unit(dtype), H.shape, B.shape[1]
    panels = (V + 31) // 32
    lse = torch.logsumexp(B, 1)
    c = (B - lse[:, None]).max(0).values
    E = float(H.abs().max()) + float(B.abs().max()) + float(lse.abs().max()) + c.abs() + 4          # [V]
    Emax = float(E.max())
    Xr, th, ph, aW = t["Xr"], t["th"], t["ph"], t["W"].abs()
    e = u * ((K + 4) + E[None] + t["logp"].abs())          # [R, V]
    vnz = (Xr > 0).sum(-1).to(F64)
    lp = RATIO * ((Xr * e).sum(-1) + (vnz + panels) * u * (Xr * t["logp"].abs()).sum(-1))
    wphi = aW @ ph.T
    td = (aW * 2 * e) @ ph.T + (vnz + panels + 4)[:, None] * u * wphi
    dH = RATIO * th * (td + u * (K + 4 + Emax) * (wphi + (g.abs() * t["N"])[:, None]))
    rnz = (Xr > 0).sum(0).to(F64)
    thw = th.T @ aW
    a = th.T @ (aW * 2 * e) + (rnz + 4)[None] * u * thw
    cs = (ph * a).sum(-1) + (V + panels + 4 + Emax) * u * (ph * t["A"].abs()).sum(-1)
    tiny = 2.0 ** -126 if dtype == F32 else 2.0 ** -1022
    dB = RATIO * (ph * (a + cs[:, None] + u * (E[None] + 4) * (t["A"].abs() + t["s"].abs()[:, None])) + tiny * (t["s"].abs()[:, None] + 2))
    return lp + 1e-300, dH + 1e-300, dB


@pytest.fixture(scope="module")
def lib():
    return load("topic")


def run(lib, dtype, ar, ops, R, K, V, Dx, splits=None):
    """prepare, logprob, grad_doc, grad_topic on the device operands ops = (H, B, X, g), any of which may be None; returns
    (return codes, lp, dH, dB)."""
    H, B, X, g = ops
    s, nb = sfx(dtype), 4 if dtype == F32 else 8
    splits = max(lib.raw("zs_topic_doc_splits", nb, R, V), 1) if splits is None else splits
    ws = [max(lib.raw("zs_topic_workspace_elems", w, nb, R, min(K, 128), V, max(Dx, 1), splits), 1) for w in range(4)]
    prep, p1, p2, p3 = (ar.out(n, dtype) for n in ws)
    lp, dH, dB = ar.out(R, dtype), ar.out(R * min(K, 128), dtype), ar.out(min(K, 128) * V, dtype)
    rcs = [lib.raw("zs_topic_prepare" + s, ptr(H), ptr(B), ptr(X), ptr(prep), R, K, V, Dx, stream()),
           lib.raw("zs_topic_logprob" + s, ptr(B), ptr(X), ptr(prep), ptr(p1), ptr(lp), R, K, V, Dx, stream()),
           lib.raw("zs_topic_grad_doc" + s, ptr(B), ptr(X), ptr(g), ptr(prep), ptr(p2), ptr(dH), R, K, V, Dx, splits, stream()),
           lib.raw("zs_topic_grad_topic" + s, ptr(B), ptr(X), ptr(g), ptr(prep), ptr(p3), ptr(dB), R, K, V, Dx, stream())]
    return rcs, lp, dH, dB


def assert_close(name, got, want, tol):
    got = got.cpu().to(F64).view(want.shape)
    err = (got - want).abs()
    ratio = float((err / tol).max())
    WORST[name.split(" [")[0]] = max(WORST.get(name.split(" [")[0], 0.0), ratio)
    print("%s: worst error / tolerance = %.3f" % (name, ratio))
    assert bool(torch.isfinite(got).all()), "%s: non-finite values" % name
    assert bool((err <= tol).all()), "%s: %d elements out of tolerance, worst error / tolerance %.3f" % (name, int((err > tol).sum()), ratio)
    return ratio


@functools.lru_cache(maxsize=2)
def case_truth(K, V, chains, docs, full):
    """the inputs of a shape and their truth, computed once and left unchanged"""
    ins = case_inputs(K, V, chains, docs, full)
    return ins, truth(*ins)


def check_case(lib, K, V, shape, full, splits=None):
    """Both element types, both layouts, twice, against the truth; `splits` = None takes the library's own zs_topic_doc_splits.
    Returns ({dtype: [lp, dH, dB] of the aligned layout, on the CPU}, {name: worst error / tolerance})."""
    (H, B, X, g), t = case_truth(K, V, shape[0], shape[1], full)
    zero_rows = (torch.arange(H.shape[0]) % X.shape[0] == 0) & (X.shape[0] > 1)
    outs, worst = {}, {}
    for dtype in (F32, F64):
        res = []
        for shift in (0, 1):
            ar = Arena(shift)
            ops = [ar.put(a, dtype) for a in (H, B, X, g)]
            dims = (H.shape[0], K, V, X.shape[0])
            first, again = run(lib, dtype, ar, ops, *dims, splits=splits), run(lib, dtype, ar, ops, *dims, splits=splits)
            ar.check_guards()
            assert first[0] == [0] * 4 and again[0] == [0] * 4
            for a, b in zip(first[1:], again[1:]):
                assert same_bits(a, b), "two identical calls differ"
            res.append([a.cpu() for a in first[1:]])
        for a, b in zip(*res):
            assert same_bits(a, b), "the aligned and the shifted layout differ"
        lp, dH, dB = res[0]
        assert bool((lp[zero_rows] == 0).all()) and bool((dH.view(H.shape)[zero_rows] == 0).all()), "an all-zero row is not exactly 0"
        tag = " [K=%d V=%d R=%d Dx=%d %s]" % (K, V, H.shape[0], X.shape[0], sfx(dtype))
        for name, got, tol in zip(("lp", "dH", "dB"), res[0], bounds(dtype, H, B, g, t)):
            worst[name + sfx(dtype)] = assert_close(name + tag, got, t[name], tol)
        outs[dtype] = res[0]
    return outs, worst


@pytest.mark.parametrize("K,V,shape,full", CASES)
def test_forward_and_backward_against_float64(lib, K, V, shape, full):
    check_case(lib, K, V, shape, full)
    print("worst error / tolerance so far: %s" % ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def test_rejected_arguments_write_nothing(lib):
    H, B, X, g = case_inputs(5, 17, 2, 3, False)
    for dtype in (F32, F64):
        ar = Arena(0)
        dh, db, dx, dg = (ar.put(a, dtype) for a in (H, B, X, g))
        assert run(lib, dtype, ar, (dh, None, dx, dg), 6, 5, 17, 3)[0] == [EINVAL] * 4          # a NULL operand
        assert run(lib, dtype, ar, (dh, db, dx, dg), 6, 5, 17, 4)[0] == [EINVAL] * 4          # R % Dx != 0
        assert run(lib, dtype, ar, (dh, db, dx, dg), 6, 129, 17, 3)[0] == [ENOTSUP] * 4          # above zs_topic_max_topics
        torch.cuda.synchronize()
        assert ar.untouched(), "a rejected call wrote something"
        rcs, _, dH, _ = run(lib, dtype, Arena(0), (dh, db, dx, dg), 6, 5, 17, 3, splits=2)          # more splits than panels
        torch.cuda.synchronize()
        assert rcs == [0, 0, EINVAL, 0] and untouched(dH)
    assert lib.raw("zs_topic_max_topics") == 128
    assert [lib.raw("zs_topic_panels", nb, v) for nb, v in ((4, 64), (4, 65), (8, 64), (8, 65), (2, 64), (4, 0))] == [1, 2, 2, 3, 0, 0]
