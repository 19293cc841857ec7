"""The mixture-of-Gaussians kernels through the raw C ABI of libzs_mix.so (include/zs_mix.h), on the GPU.  See
tests/README_mix.md.

Truth: the definition in float64 torch on the CPU (``truth`` below: the broadcast (x - mean)^2 form, ``torch.logsumexp``,
``autograd.grad``), on float32-representable inputs, so one truth serves _f32 and _f64.  Every case runs with aligned operands and
with every operand shifted by one element: the two must agree bit for bit, the guard elements around every operand, output and
workspace must survive, and the same calls twice must give the same bits.

Inputs, keyed on the shape.  mean = shift + 2 N(0,1) with shift one of {0, +30, -30}; logstd = -1 + 0.5 N(0,1); logits =
offset + 3 N(0,1) with offset one of {-80, 0, +80} and component C // 2 lowered by 90 (C > 1); x = shift + N(0,1) with row 0
moved 100 away (R > 1); g ~ N(0,1).

Tolerances (derived, not tuned; the worst error / bound the MI355X gave is recorded in README_mix.md; u = 2^-24 for _f32, 2^-53
for _f64; RATIO = 4 as in README_topic.md; tiny = the smallest normal number: a value below it is flushed or held to the
subnormal spacing).  With w = exp(-2 logstd), the centre m, y = x - m, nu = mean - m (the centre cancels exactly whatever its own
rounding, as y and nu read the same m), E_w = 2 max|logstd| + 4 roundings in w (the argument, the exponential) and r = the truth's
responsibilities exp(s - lp):
  e_b[c]   = u [ 2 (max|logits| + |lsm_c|) + C + 4 + (D + 1) sum_d |logstd| + D log 2 pi + (D + E_w + 4) q_c + 4 |b_c| ]
             log_softmax over C terms, the D-term sums, q_c = 1/2 sum_d w nu^2, the final additions
  e_s[r,c] = u (2 D + 4 + E_w) P_rc + e_b[c] + 2 u |s_rc|         P_rc = sum_d |y w nu| + 1/2 y^2 w, what the expanded product adds:
             each of its 2 D terms carries (4 + E_w) u, the accumulation 2 D u
  lp       e_lp[r] = sum_c r e_s + u [ C / 4 + 12 + 2 sum_c r |s - max s| + 2 |lp| ]      a lane adds C / 16 exponentials, four lanes
             combine; exp2(x log2 e) carries 2 |x| u
  G        e_G[r,c] = |g| min( r expm1(e_s + e_lp + u (4 + 2 |s - lp|)), 1 ) + tiny |g|      (a responsibility stays within [0, 1])
  n        e_n[c] = sum_r e_G + (R + 20) u sum_r |G|              at most R roundings over the rows, the shares, the finish
  dx       sum_c e_G (|w nu| + |y| w) + u (C + E_w + 8) sum_c |G| (|w nu| + |y| w)
  GY, GY2  e_GY = sum_r e_G |y| + (R + 22) u sum_r |G y| ; likewise with y^2
  dmean    w [ e_GY + |nu| e_n + u (E_w + 6) (sum|G y| + |nu| sum|G|) ]
  dlogstd  w [ e_GY2 + 2 |nu| e_GY + nu^2 e_n ] + e_n + u (E_w + 8) [ w (sum|G y^2| + 2 |nu| sum|G y| + nu^2 sum|G|) + sum|G| ]
  dlogits  e_n + u (R + 24 + C + 2 (max|logits| + |lsm|)) (sum|G| + pi_c sum|g|) + tiny (sum|g| + 2)
each times RATIO, the gradients plus 2 tiny."""
import functools
import math

import numpy as np
import pytest
import torch

from kernel_abi import EINVAL, ENOTSUP, F32, F64, Arena, load, ptr, same_bits, sfx, stream, unit, untouched

pytestmark = pytest.mark.gpu

RATIO = 4
DS = [1, 3, 4, 5, 40, 64]
CS = [1, 15, 16, 17, 65, 500]
RS = [1, 17, 33, 130]
# a cycling subset of the product: every D and every C twice, every R three times, (D, C, R) = (64, 500, 130) at i = 5
CASES = [(DS[i % 6], CS[(i + i // 6) % 6], RS[(i + 2) % 4]) for i in range(12)]
NAMES = ("lp", "dx", "dlogits", "dmean", "dlogstd")
WORST = {}          # quantity -> the worst error / tolerance seen in this session (printed; recorded in README_mix.md)


def f32r(a):
    return torch.from_numpy(np.asarray(a).astype(np.float32).astype(np.float64))


def case_inputs(D, C, R):
    """(logits [C], mean [C, D], logstd [C, D], x [R, D], g [R]) in float64, float32-representable"""
    rng = np.random.default_rng(100000 * D + 100 * C + R)
    shift, offset = (0.0, 30.0, -30.0)[(D + C + R) % 3], (-80.0, 0.0, 80.0)[(D + C) % 3]
    logits = offset + 3.0 * rng.standard_normal(C)
    if C > 1:
        logits[C // 2] -= 90.0
    x = shift + rng.standard_normal((R, D))
    if R > 1:
        x[0] += 100.0
    return (f32r(logits), f32r(shift + 2.0 * rng.standard_normal((C, D))), f32r(-1.0 + 0.5 * rng.standard_normal((C, D))), f32r(x),
            f32r(rng.standard_normal(R)))


def truth(logits, mean, logstd, x, g):
    """lp, the four gradients of sum(g lp) and the component scores, in float64, from the definition"""
    ps = [t.clone().requires_grad_(True) for t in (x, logits, mean, logstd)]
    xx, lg, mu, ls = ps
    s = (-0.5 * ((xx[:, None, :] - mu) / torch.exp(ls)) ** 2 - ls - 0.5 * math.log(2 * math.pi)).sum(-1) + torch.log_softmax(lg, 0)
    lp = torch.logsumexp(s, 1)
    grads = torch.autograd.grad((lp * g).sum(), ps)
    return dict(zip(NAMES, (lp.detach(),) + grads), s=s.detach())


def bounds(dtype, logits, mean, logstd, x, g, t):
    """the five tolerances of the docstring, in the order of NAMES"""
    u, (C, D), R = unit(dtype), mean.shape, x.shape[0]
    tiny = 2.0 ** -126 if dtype == F32 else 2.0 ** -1022
    w, cen = torch.exp(-2 * logstd), mean.mean(0)
    y, nu, Ew, lmax = (x - cen).abs(), (mean - cen).abs(), 2 * float(logstd.abs().max()) + 4, float(logits.abs().max())
    lsm, q = torch.log_softmax(logits, 0), 0.5 * (w * nu * nu).sum(-1)
    b = lsm - logstd.sum(-1) - 0.5 * D * math.log(2 * math.pi) - q
    eb = u * (2 * (lmax + lsm.abs()) + C + 4 + (D + 1) * logstd.abs().sum(-1) + D * math.log(2 * math.pi) + (D + Ew + 4) * q + 4 * b.abs())
    s, lp, ag = t["s"], t["lp"], g.abs()
    es = u * (2 * D + 4 + Ew) * (y @ (w * nu).T + 0.5 * (y * y) @ w.T) + eb[None] + 2 * u * s.abs()
    r = torch.exp(s - lp[:, None])
    elp = (r * es).sum(1) + u * (C / 4 + 12 + 2 * (r * (s - s.max(1, keepdim=True).values).abs()).sum(1) + 2 * lp.abs())
    eG = ag[:, None] * torch.clamp(r * torch.expm1(es + elp[:, None] + u * (4 + 2 * (s - lp[:, None]).abs())), max=1.0) + tiny * ag[:, None]
    aG = ag[:, None] * r
    en, n = eG.sum(0) + (R + 20) * u * aG.sum(0), aG.sum(0)
    edx = eG @ (w * nu) + y * (eG @ w) + u * (C + Ew + 8) * (aG @ (w * nu) + y * (aG @ w))
    GY, GY2 = aG.T @ y, aG.T @ (y * y)
    eGY, eGY2 = eG.T @ y + (R + 22) * u * GY, eG.T @ (y * y) + (R + 22) * u * GY2
    edmean = w * (eGY + nu * en[:, None] + u * (Ew + 6) * (GY + nu * n[:, None]))
    edlogstd = (w * (eGY2 + 2 * nu * eGY + nu * nu * en[:, None]) + en[:, None]
                + u * (Ew + 8) * (w * (GY2 + 2 * nu * GY + nu * nu * n[:, None]) + n[:, None]))
    edlogits = en + u * (R + 24 + C + 2 * (lmax + lsm.abs())) * (n + torch.exp(lsm) * ag.sum()) + tiny * (ag.sum() + 2)
    return [RATIO * elp] + [RATIO * e + 2 * tiny for e in (edx, edlogits, edmean, edlogstd)]


@pytest.fixture(scope="module")
def lib():
    return load("mix")


def run(lib, dtype, ar, ops, R, C, D, shares=None):
    """prepare, logprob, grad_x, grad_params on the device operands ops = (logits, mean, logstd, x, g), any of which may be None;
    returns (return codes, [lp, dx, dlogits, dmean, dlogstd])."""
    logits, mean, logstd, x, g = (ptr(o) for o in ops)
    s, nb, Dc = sfx(dtype), 4 if dtype == F32 else 8, min(D, 64)
    shares = max(lib.raw("zs_mix_row_shares", nb, R, C), 1) if shares is None else shares
    prep, part = (ar.out(max(lib.raw("zs_mix_workspace_elems", k, nb, C, Dc, max(shares, 1)), 1), dtype) for k in (0, 1))
    outs = [ar.out(n, dtype) for n in (R, R * Dc, C, C * Dc, C * Dc)]
    lp, dx, dlogits, dmean, dlogstd = (ptr(o) for o in outs)
    rcs = [lib.raw("zs_mix_prepare" + s, logits, mean, logstd, ptr(prep), C, D, stream()),
           lib.raw("zs_mix_logprob" + s, x, ptr(prep), lp, R, C, D, stream()),
           lib.raw("zs_mix_grad_x" + s, x, g, lp, ptr(prep), dx, R, C, D, stream()),
           lib.raw("zs_mix_grad_params" + s, x, g, lp, mean, logstd, ptr(prep), ptr(part), dlogits, dmean, dlogstd, R, C, D, shares, stream())]
    return rcs, outs


def assert_close(name, got, want, tol):
    got = got.detach().cpu().to(F64).reshape(want.shape)
    err = (got - want).abs()
    ratio = float((err / tol).max())
    WORST[name.split(" [")[0]] = max(WORST.get(name.split(" [")[0], 0.0), ratio)
    print("%s: worst error / tolerance = %.3f" % (name, ratio))
    assert bool(torch.isfinite(got).all()), "%s: non-finite values" % name
    assert bool((err <= tol).all()), "%s: %d elements out of tolerance, worst error / tolerance %.3f" % (name, int((err > tol).sum()), ratio)
    return ratio


@functools.lru_cache(maxsize=2)
def case_truth(D, C, R):
    """the inputs of a shape and their truth, computed once and left unchanged"""
    ins = case_inputs(D, C, R)
    return ins, truth(*ins)


def check_case(lib, D, C, R, shares=None):
    """Both element types, both layouts, twice, against the truth; `shares` = None takes the library's own zs_mix_row_shares.
    Returns ({dtype: [lp, dx, dlogits, dmean, dlogstd] of the aligned layout, on the CPU}, {name: worst error / tolerance})."""
    ins, t = case_truth(D, C, R)
    outs, worst = {}, {}
    for dtype in (F32, F64):
        res = []
        for shift in (0, 1):
            ar = Arena(shift)
            ops = [ar.put(a, dtype) for a in ins]
            first, again = run(lib, dtype, ar, ops, R, C, D, shares), run(lib, dtype, ar, ops, R, C, D, shares)
            ar.check_guards()
            assert first[0] == [0] * 4 and again[0] == [0] * 4
            for a, b in zip(first[1], again[1]):
                assert same_bits(a, b), "two identical calls differ"
            res.append([a.cpu() for a in first[1]])
        for a, b in zip(*res):
            assert same_bits(a, b), "the aligned and the shifted layout differ"
        tag, tols = " [D=%d C=%d R=%d %s]" % (D, C, R, sfx(dtype)), bounds(dtype, *ins, t)
        for name, got, tol in zip(NAMES, res[0], tols):
            worst[name + sfx(dtype)] = assert_close(name + tag, got, t[name], tol)          # (finite too: the lowered component's rows, the far row)
        if C == 1:
            plain = torch.distributions.Normal(ins[1][0], torch.exp(ins[2][0])).log_prob(ins[3]).sum(-1)
            assert_close("lp against the diagonal normal" + tag, res[0][0], plain, tols[0])
        outs[dtype] = res[0]
    return outs, worst


@pytest.mark.parametrize("D,C,R", CASES)
def test_forward_and_backward_against_float64(lib, D, C, R):
    check_case(lib, D, C, R)
    print("worst error / tolerance so far: %s" % ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def test_rejected_arguments_write_nothing(lib):
    ins = case_inputs(5, 17, 33)
    for dtype in (F32, F64):
        ar = Arena(0)
        ops = [ar.put(a, dtype) for a in ins]
        rcs, outs = run(lib, dtype, ar, ops[:3] + [None, ops[4]], 33, 17, 5)          # a NULL operand (prepare does not take x)
        assert rcs == [0, EINVAL, EINVAL, EINVAL]
        rcs65, outs65 = run(lib, dtype, ar, ops, 33, 17, 65)          # above zs_mix_max_dim
        assert rcs65 == [ENOTSUP] * 4
        for shares in (0, 4):          # 33 rows are three strips of 16
            rcs_s, outs_s = run(lib, dtype, ar, ops, 33, 17, 5, shares=shares)
            assert rcs_s == [0, 0, 0, EINVAL]
            outs += outs_s[2:]
        torch.cuda.synchronize()
        assert all(untouched(o) for o in outs + outs65), "a rejected call wrote something"
        ar.check_guards()
    assert (lib.raw("zs_mix_max_dim"), lib.raw("zs_mix_max_components")) == (64, 65536)
    assert [lib.raw("zs_mix_panels", nb, c) for nb, c in ((4, 64), (4, 65), (8, 64), (8, 65), (2, 64), (4, 0))] == [1, 2, 2, 3, 0, 0]
    assert [lib.raw("zs_mix_row_shares", 4, r, c) for r, c in ((1, 1), (130, 16), (102400, 500), (0, 5))] == [1, 9, 64, 0]
