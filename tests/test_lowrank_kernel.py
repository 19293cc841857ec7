"""The low-rank multivariate-normal kernels through the raw C ABI of libzs_lowrank.so (include/zs_lowrank.h), on the GPU.  See
tests/README_lowrank.md.

Truth: the definition in float64 torch on the CPU -- ``torch.distributions.MultivariateNormal(mean, diag(d) + W W^T)`` and
``autograd.grad`` of ``sum(g lp)``; the draw and its gradients from ``mean + sqrt(d) eps_D + W eps_r`` -- on float32-representable
inputs, so one truth serves _f32 and _f64.  Every case runs with aligned operands and with every operand shifted by one element:
the two must agree bit for bit, the guard elements around every operand, output and workspace must survive, and the same calls
twice must give the same bits.  Every case runs with the D-splits of the prepare and the particle shares of the backward forced
to 1 and with the library's own counts (zs_lowrank_splits); both are held to the truth.

Inputs, keyed on the shape: d in [0.3, 1.3], W = N(0,1) / sqrt(r), mean = shift + N(0,1) with shift one of {0, +30, -30},
x = mean + 1.5 N(0,1) with one row moved 100 away, g, gz, eps ~ N(0,1).  Every other case with K > 1 hands the kernels a value
without the particle axis (Px = R D).

Tolerances (u = 2^-24 for _f32, 2^-53 for _f64; RATIO = 4 as in README_topic.md).  The draw and its gradients have rounding
bounds from their operation counts:
  z        u (r + 4) (|mean| + sqrt(d) |eps_D| + |E_r| |W|^T)          r products and additions, the square root, two additions
  gmean    u (K + 2) sum_k |gz|
  gfactor  u (K + 2) |Gz|^T |E_r|
  gdiag    u (K + 6) sum_k |gz eps_D| / (2 sqrt d)
each times RATIO.  The density goes through a Cholesky factorisation of the capacitance and the Woodbury difference
sum y^2 / d - u C^-1 u^T, whose cancellation depends on the inputs: no bound from operation counts is derived.  lp, gx, gmean,
gfactor and gdiag are held, per tensor in the maximum norm, to 16 x the error of the torch Woodbury composition
(zhusuan.distributions._lowrank_functions.torch_log_prob, on the CPU, in the element type of the kernel) against the same truth,
plus the floor of tests/test_gradcheck.py, 4 u max|truth|.  (A floor of u max|truth| alone is half a unit in the last place of
the largest element: where the composition happens to round exactly -- D = r = K = 1, |lp| = 12544 in _f64 -- no sum in another
order can meet it; that case gave 1.3 of such a bound with an error of one unit in the last place.)"""
import functools

import numpy as np
import pytest
import torch

from kernel_abi import DEV, EINVAL, ENOTSUP, F32, F64, I64, Arena, load, load_main, ptr, same_bits, sfx, stream, unit, untouched

pytestmark = pytest.mark.gpu

RATIO = 4
DS = [1, 15, 16, 17, 65, 150]          # 65: one panel + 1; 150: three panels, so three D-splits
RANKS = [1, 4, 5, 16, 17, 64]
KS = [1, 17, 33]
RS = [1, 3]
# a cycling subset of the product: every D and every rank twice, (D, r) = (150, 64) at i = 5
CASES = [(DS[i % 6], RANKS[(i + i // 6) % 6], KS[(i + i // 6) % 3], RS[(i // 3) % 2], i % 2 == 1) for i in range(12)]
DENSITY = ("lp", "gx", "gmean", "gfactor", "gdiag")
DRAW = ("z", "s_gmean", "s_gfactor", "s_gdiag")
WORST = {}          # quantity -> the worst error / tolerance seen in this session (printed; recorded in README_lowrank.md)


def f32r(a):
    return torch.from_numpy(np.asarray(a).astype(np.float32).astype(np.float64))


def case_inputs(D, r, K, R):
    """(mean [R, D], W [R, D, r], d [R, D], x [K, R, D], g [K, R], eps [K, R, D + r], gz [K, R, D]) in float64,
    float32-representable"""
    rng = np.random.default_rng(1000000 * D + 10000 * r + 100 * K + R)
    mean = (0.0, 30.0, -30.0)[(D + r + K) % 3] + rng.standard_normal((R, D))
    x = mean + 1.5 * rng.standard_normal((K, R, D))
    x[K - 1, 0] += 100.0
    return tuple(f32r(a) for a in (mean, rng.standard_normal((R, D, r)) / np.sqrt(r), 0.3 + rng.random((R, D)), x,
                                   rng.standard_normal((K, R)), rng.standard_normal((K, R, D + r)), rng.standard_normal((K, R, D))))


def density(fn, mean, W, d, x, g, dtype):
    """lp of fn and the gradients of sum(g lp) for (x, mean, W, d), in `dtype` on the CPU, returned in float64"""
    ps = [t.to(dtype).clone().requires_grad_(True) for t in (x, mean, W, d)]
    lp = fn(ps[1], ps[2], ps[3], ps[0])
    grads = torch.autograd.grad((lp * g.to(dtype)).sum(), ps)
    return dict(zip(DENSITY, [t.detach().to(F64) for t in (lp,) + grads]))


def mvn_log_prob(mean, W, d, x):
    return torch.distributions.MultivariateNormal(mean, torch.diag_embed(d) + W @ W.transpose(-1, -2)).log_prob(x)


@functools.lru_cache(maxsize=2)
def case_truth(D, r, K, R, shared):
    """the inputs of a shape, their truth, the tolerances of both element types: computed once and left unchanged"""
    from zhusuan.distributions._lowrank_functions import torch_log_prob
    ins = case_inputs(D, r, K, R)
    mean, W, d, x, g, eps, gz = ins
    if shared:
        x = x[:1].expand(K, R, D).contiguous()
        ins = (mean, W, d, x, g, eps, gz)
    t = density(mvn_log_prob, mean, W, d, x, g, F64)
    eD, eR = eps[..., :D], eps[..., D:]
    t.update(z=mean + torch.sqrt(d) * eD + (W @ eR[..., None])[..., 0], s_gmean=gz.sum(0), s_gfactor=torch.einsum("krd,krj->rdj", gz, eR),
             s_gdiag=(gz * eD).sum(0) / (2 * torch.sqrt(d)))
    tols = {}
    for dtype in (F32, F64):
        u, comp = unit(dtype), density(torch_log_prob, mean, W, d, x, g, dtype)
        tol = dict((n, 16 * float((comp[n] - t[n]).abs().max()) + 4 * u * float(t[n].abs().max())) for n in DENSITY)
        tol["z"] = RATIO * u * (r + 4) * (mean.abs() + torch.sqrt(d) * eD.abs() + (W.abs() @ eR.abs()[..., None])[..., 0])
        tol["s_gmean"] = RATIO * u * (K + 2) * gz.abs().sum(0)
        tol["s_gfactor"] = RATIO * u * (K + 2) * torch.einsum("krd,krj->rdj", gz.abs(), eR.abs())
        tol["s_gdiag"] = RATIO * u * (K + 6) * (gz * eD).abs().sum(0) / (2 * torch.sqrt(d))
        tols[dtype] = tol
    return ins, t, tols


@pytest.fixture(scope="module")
def lib():
    return load("lowrank")


def counts(lib, K, R, D):
    return tuple(max(lib.raw("zs_lowrank_splits", which, K, R, D), 1) for which in (1, 2))


def run(lib, dtype, ar, ops, K, R, D, r, n=(1, 1), shared=False, seed=0, call=0, rs=None):
    """prepare, logprob, logprob_bwd, sample, sample_bwd on the device operands ops = (mean, W, d, x, g, eps, gz), any of which
    may be None; n = (D-splits, particle shares).  Returns (return codes, the nine outputs in the order DENSITY + DRAW)."""
    mean, W, d, x, g, eps, gz = (ptr(o) for o in ops)
    s, Dc, rc = sfx(dtype), min(D, 150), min(r, 64)
    ws = [ar.out(max(lib.raw("zs_lowrank_workspace_elems", which, R, Dc, rc, k), 1), dtype) for which, k in ((0, 1), (1, n[0]), (2, n[1]))]
    prep, part, bpart = (ptr(w) for w in ws)
    outs = [ar.out(k, dtype) for k in (K * R, K * R * Dc, R * Dc, R * Dc * rc, R * Dc, K * R * Dc, R * Dc, R * Dc * rc, R * Dc)]
    lp, gx, gmean, gW, gd, z, sgmean, sgW, sgd = (ptr(o) for o in outs)
    Px = (R if shared else K * R) * D
    rcs = [lib.raw("zs_lowrank_prepare" + s, W, d, part, prep, R, D, r, n[0], stream()),
           lib.raw("zs_lowrank_logprob" + s, mean, W, d, prep, x, Px, lp, K, R, D, r, stream()),
           lib.raw("zs_lowrank_logprob_bwd" + s, mean, W, d, prep, x, Px, g, bpart, gx, gmean, gW, gd, K, R, D, r, n[1], stream()),
           lib.raw("zs_lowrank_sample" + s, mean, W, d, eps, z, K, R, D, r, seed, call, ptr(rs), stream()),
           lib.raw("zs_lowrank_sample_bwd" + s, d, eps, gz, sgmean, sgW, sgd, K, R, D, r, seed, call, ptr(rs), stream())]
    return rcs, outs


def assert_close(name, got, want, tol):
    got = got.detach().cpu().to(F64).reshape(want.shape)
    err = (got - want).abs()
    ratio = float((err / tol).max())
    key = name.split(" [")[0]
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print("%s: worst error / tolerance = %.3f" % (name, ratio))
    assert bool(torch.isfinite(got).all()), "%s: non-finite values" % name
    assert bool((err <= tol).all()), "%s: %d elements out of tolerance, worst error / tolerance %.3f" % (name, int((err > tol).sum()), ratio)


@pytest.mark.parametrize("D,r,K,R,shared", CASES)
def test_density_and_draw_against_float64(lib, D, r, K, R, shared):
    shared = shared and K > 1
    ins, t, tols = case_truth(D, r, K, R, shared)
    for dtype in (F32, F64):
        for n in ((1, 1), counts(lib, K, R, D)):
            res = []
            for shift in (0, 1):
                ar = Arena(shift)
                ops = [ar.put(a, dtype) for a in ins]
                if shared:
                    ops[3] = ar.put(ins[3][0], dtype)
                first, again = run(lib, dtype, ar, ops, K, R, D, r, n, shared), run(lib, dtype, ar, ops, K, R, D, r, n, shared)
                ar.check_guards()
                assert first[0] == [0] * 5 and again[0] == [0] * 5
                for a, b in zip(first[1], again[1]):
                    assert same_bits(a, b), "two identical calls differ"
                res.append([a.cpu() for a in first[1]])
            for a, b in zip(*res):
                assert same_bits(a, b), "the aligned and the shifted layout differ"
            tag = " [D=%d r=%d K=%d R=%d n=%s %s]" % (D, r, K, R, n, sfx(dtype))
            for name, got in zip(DENSITY + DRAW, res[0]):
                assert_close(name + sfx(dtype) + tag, got, t[name], tols[dtype][name])
    print("worst error / tolerance so far: %s" % ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def test_philox_draw_equals_the_injected_stream(lib):
    """eps = NULL draws element (k R + row) (D + r) + j of zs_philox_normal's stream: the draw and its backward equal, bit for
    bit, the calls fed that stream as `eps`."""
    D, r, K, R = 65, 5, 17, 3
    ins = case_inputs(D, r, K, R)
    n = K * R * (D + r)
    for dtype in (F32, F64):
        for seed, call, state in ((11, 3, None), (0, 2, (77, 1 << 33))):
            rs = None if state is None else torch.tensor(state, dtype=I64, device=DEV)
            noise = torch.empty(n, dtype=F32, device=DEV)
            load_main().call("zs_philox_normal_f32", noise.data_ptr(), n, seed, call, ptr(rs), stream())
            ar = Arena(1)
            ops = [ar.put(a, dtype) for a in ins]
            drawn = run(lib, dtype, ar, ops[:5] + [None, ops[6]], K, R, D, r, seed=seed, call=call, rs=rs)
            ops[5] = ar.put(noise.cpu().reshape(K, R, D + r), dtype)
            fed = run(lib, dtype, ar, ops, K, R, D, r)
            ar.check_guards()
            assert drawn[0] == [0] * 5 and fed[0] == [0] * 5
            for a, b in zip(drawn[1][5:], fed[1][5:]):
                assert same_bits(a, b), "the in-kernel stream differs from zs_philox_normal"


def test_rejected_arguments_write_nothing(lib):
    D, r, K, R = 17, 5, 17, 3
    ins = case_inputs(D, r, K, R)
    cap = lib.raw("zs_lowrank_max_dim")
    assert (cap, lib.raw("zs_lowrank_max_rank")) == (65536, 64) and cap >= 16384
    for dtype in (F32, F64):
        ar = Arena(0)
        ops = [ar.put(a, dtype) for a in ins]
        outs = []
        for rr, DD, want in ((65, D, ENOTSUP), (r, cap + 1, ENOTSUP), (0, D, EINVAL)):
            rcs, o = run(lib, dtype, ar, ops, K, R, DD, rr)
            assert rcs == [want] * 5
            outs += o
        rcs, o = run(lib, dtype, ar, [None] + ops[1:], K, R, D, r)          # a NULL operand (prepare and sample_bwd do not take mean)
        assert rcs == [0, EINVAL, EINVAL, EINVAL, 0]
        outs += o[:6]
        for n, want in (((2, 1), [EINVAL, 0, 0]), ((1, 3), [0, 0, EINVAL]), ((0, 0), [EINVAL, 0, EINVAL])):          # D = 17 is one panel, K = 17 two tiles
            rcs, o = run(lib, dtype, ar, ops, K, R, D, r, n)
            assert rcs[:3] == want
            outs += [o[i] for i in range(5) if (rcs[2] if i else rcs[1]) != 0]
        torch.cuda.synchronize()
        assert all(untouched(o) for o in outs), "a rejected call wrote something"
        ar.check_guards()
    assert [lib.raw("zs_lowrank_splits", 1, 0, R, D) for R, D in ((1, 64), (1, 150), (1, 65536), (400, 65536), (0, 5))] == [1, 3, 512, 2, 0]
    assert [lib.raw("zs_lowrank_splits", 2, K, R, 5) for K, R in ((1, 1), (33, 1), (33, 400), (10000, 2), (0, 1))] == [1, 3, 2, 256, 0]
