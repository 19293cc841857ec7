"""The sparse-GP conditional kernels through the raw C ABI of libzs_gp.so (include/zs_gp.h), on the GPU.  See tests/README_gp.md.

Truth: the definition in float64 torch on the CPU -- explicit differences for k(x, Z), ``solve_triangular`` for A = L^-1 k(Z, x)
and L^-1 fz, ``autograd.grad`` of ``sum(gmean mean) + sum(gvar var)`` -- on float32-representable inputs, so one truth serves _f32
and _f64.  The upper triangle of the factor handed to the kernels is NaN.  Every case runs with fz with and without the particle
axis, with aligned operands and with every operand shifted by one element (the two must agree bit for bit, and the guard elements
must survive), twice (the same bits), and with the row shares forced to 1 and with zs_gp_row_shares' count.

Inputs, keyed on the shape: lengthscales in [0.7, 1.4], amplitude 1.3, inducing inputs on a lattice 1.25 lengthscales apart over the
first min(d, 3) dimensions, moved by at most 0.05 lengthscales; x = a random inducing input + 0.5 lengthscales N(0, 1); the factor is the
Cholesky factor of k(Z, Z) + 0.1 a^2 I.  The truth's var >= 0.05 a^2 is asserted: otherwise the tolerance would measure the
conditioning of L.

Tolerance: per tensor in the maximum norm, 16 x the error of the torch composition
(zhusuan.distributions._gp_functions.torch_moments, on the CPU, in the element type of the kernel) against the same truth, plus
the floor of tests/test_gradcheck.py, 4 u max|truth|."""
import functools

import numpy as np
import pytest
import torch

from kernel_abi import EINVAL, ENOTSUP, F32, F64, Arena, load, ptr, same_bits, sfx, stream, unit, untouched

pytestmark = pytest.mark.gpu

# (N, M, d, K); N = 150 is three 64-row blocks, so three shares; M = 128 is float32 only
CASES = [(1, 1, 1, 1), (17, 15, 3, 5), (33, 16, 5, 17), (17, 17, 64, 1), (33, 33, 1, 5), (17, 64, 3, 17), (33, 128, 5, 5),
         (1, 17, 5, 17), (33, 15, 64, 5), (17, 33, 3, 1), (33, 64, 64, 17), (17, 16, 1, 5), (150, 17, 3, 5), (150, 64, 5, 17),
         (150, 128, 64, 5)]
NAMES = ("mean", "var", "gx", "gZ", "glen", "gamp", "gL", "gfz")
AMP = 1.3


def f32r(a):
    return torch.from_numpy(np.asarray(a).astype(np.float32).astype(np.float64))


def case_inputs(N, M, d, K):
    """(x [N, d], Z [M, d], l [d], a [1], L [M, M], fz [K, M], gmean [K, N], gvar [N]) in float64, float32-representable"""
    rng = np.random.default_rng(1000000 * N + 10000 * M + 100 * d + K)
    dims = min(d, 3)
    side = int(np.ceil(M ** (1.0 / dims)))
    l = 0.7 + 0.7 * rng.random(d)
    grid = np.zeros((M, d))
    for j in range(dims):
        grid[:, j] = (np.arange(M) // side ** j) % side
    Z = f32r((1.25 * grid + 0.1 * (rng.random((M, d)) - 0.5)) * l)
    x = f32r(Z.numpy()[rng.integers(0, M, N)] + 0.5 * l * rng.standard_normal((N, d)))
    l, a = f32r(l), f32r([AMP])
    diff = (Z[:, None, :] - Z[None, :, :]) / l
    L = f32r(torch.linalg.cholesky(a ** 2 * torch.exp(-0.5 * (diff * diff).sum(-1)) + 0.1 * a ** 2 * torch.eye(M, dtype=F64)).numpy())
    return x, Z, l, a, L, f32r(rng.standard_normal((K, M))), f32r(rng.standard_normal((K, N))), f32r(rng.standard_normal(N))


def defined_moments(x, Z, l, a, L, fz):
    diff = (x[:, None, :] - Z[None, :, :]) / l
    kxz = a ** 2 * torch.exp(-0.5 * (diff * diff).sum(-1))
    A = torch.linalg.solve_triangular(torch.tril(L), kxz.t(), upper=False)
    w = torch.linalg.solve_triangular(torch.tril(L), fz.t(), upper=False)
    return w.t() @ A, a ** 2 - (A * A).sum(0)


def evaluate(fn, ins, dtype):
    """the moments of fn and the gradients of sum(gmean mean) + sum(gvar var), in `dtype` on the CPU, returned in float64"""
    ps = [t.to(dtype).clone().requires_grad_(True) for t in ins[:6]]
    mean, var = fn(*ps)
    grads = torch.autograd.grad((mean * ins[6].to(dtype)).sum() + (var * ins[7].to(dtype)).sum(), ps)
    return dict(zip(NAMES, [t.detach().to(F64) for t in (mean, var) + grads]))


@functools.lru_cache(maxsize=2)
def case_truth(N, M, d, K, shared):
    """the inputs of a shape, their truth, the tolerances of both element types: computed once and left unchanged"""
    from zhusuan.distributions._gp_functions import torch_moments
    ins = case_inputs(N, M, d, K)
    if shared:
        ins = ins[:5] + (ins[5][:1],) + ins[6:]          # fz [1, M] broadcasts over the K rows of gmean: gfz sums over them
        fn = [lambda *p, f=f: f(*p[:5], p[5].expand(K, M)) for f in (defined_moments, torch_moments)]
    else:
        fn = [defined_moments, torch_moments]
    t = evaluate(fn[0], ins, F64)
    assert float(t["var"].min()) >= 0.05 * AMP ** 2, "the inputs are too close to the inducing inputs for the jitter"
    tols = {}
    for dtype in (F32, F64):
        comp = evaluate(fn[1], ins, dtype)
        tols[dtype] = dict((n, 16 * float((comp[n] - t[n]).abs().max()) + 4 * unit(dtype) * float(t[n].abs().max())) for n in NAMES)
    return ins, t, tols


@pytest.fixture(scope="module")
def lib():
    return load("gp")


def run(lib, dtype, ar, ops, N, M, d, K, shares=1, shared=False, null=()):
    """prepare, moments, moments_bwd on the device operands ops = (x, Z, l, a, L, fz, gmean, gvar), any of which may be None;
    the backward gets NULL for the outputs named in `null`.  Returns (return codes, the eight outputs in the order NAMES)."""
    x, Z, l, a, L, fz, gmean, gvar = (ptr(o) for o in ops)
    s, Mc, dc = sfx(dtype), min(M, 128), min(d, 64)
    ws = [ar.out(max(lib.raw("zs_gp_workspace_elems", which, Mc, dc, K, n), 1), dtype) for which, n in ((0, 1), (1, max(shares, 1)))]
    prep, part = (ptr(w) for w in ws)
    outs = [ar.out(k, dtype) for k in (K * N, N, N * dc, Mc * dc, dc, 1, Mc * Mc, (1 if shared else K) * Mc)]
    mean, var, gx, gZ, gl, ga, gL, gfz = (None if n in null else ptr(o) for n, o in zip(NAMES, outs))
    Pf = (1 if shared else K) * M
    rcs = [lib.raw("zs_gp_prepare" + s, L, fz, Pf, prep, M, K, stream()),
           lib.raw("zs_gp_moments" + s, x, Z, l, a, prep, mean, var, N, M, d, K, stream()),
           lib.raw("zs_gp_moments_bwd" + s, x, Z, l, a, Pf, prep, gmean, gvar, part, gx, gZ, gl, ga, gL, gfz, N, M, d, K, shares, stream())]
    return rcs, outs


def assert_close(name, got, want, tol):
    got = got.detach().cpu().to(F64).reshape(want.shape)
    ratio = float((got - want).abs().max()) / tol
    assert bool(torch.isfinite(got).all()), "%s: non-finite values" % name
    assert ratio <= 1.0, "%s: worst error / tolerance %.3f" % (name, ratio)


@pytest.mark.parametrize("N,M,d,K", CASES)
def test_moments_and_gradients_against_float64(lib, N, M, d, K):
    for shared in ((False, True) if K > 1 else (False,)):
        ins, t, tols = case_truth(N, M, d, K, shared)
        L = ins[4] + torch.triu(torch.full((M, M), float("nan"), dtype=F64), 1)
        for dtype in ((F32, F64) if M <= 64 else (F32,)):
            for shares in sorted({1, max(lib.raw("zs_gp_row_shares", N), 1)}):
                res = []
                for shift in (0, 1):
                    ar = Arena(shift)
                    ops = [ar.put(a, dtype) for a in ins[:4] + (L,) + ins[5:]]
                    if shared:
                        ops[5] = ar.put(ins[5][0], dtype)
                    first, again = (run(lib, dtype, ar, ops, N, M, d, K, shares, shared) for _ in range(2))
                    ar.check_guards()
                    assert first[0] == [0] * 3 and again[0] == [0] * 3
                    for a, b in zip(first[1], again[1]):
                        assert same_bits(a, b), "two identical calls differ"
                    res.append([a.cpu() for a in first[1]])
                for a, b in zip(*res):
                    assert same_bits(a, b), "the aligned and the shifted layout differ"
                tag = " [N=%d M=%d d=%d K=%d shares=%d shared=%d %s]" % (N, M, d, K, shares, shared, sfx(dtype))
                assert not bool(res[0][6].reshape(M, M).triu(1).ne(0).any()), "gL above the diagonal is not zero"
                for name, got in zip(NAMES, res[0]):
                    assert_close(name + sfx(dtype) + tag, got, t[name], tols[dtype][name])


def test_null_gradients_and_outputs(lib):
    """gmean or gvar NULL is a zero gradient; outputs that are NULL are not written and leave the others' bits unchanged"""
    N, M, d, K = 33, 17, 3, 5
    ins, t, _ = case_truth(N, M, d, K, False)
    for dtype in (F32, F64):
        ar = Arena(1)
        ops = [ar.put(a, dtype) for a in ins]
        zero = [ar.put(torch.zeros_like(a), dtype) for a in ins[6:]]
        full = run(lib, dtype, ar, ops, N, M, d, K)
        for i in (6, 7):
            null = run(lib, dtype, ar, ops[:i] + [None] + ops[i + 1:], N, M, d, K)
            zeroed = run(lib, dtype, ar, ops[:i] + [zero[i - 6]] + ops[i + 1:], N, M, d, K)
            assert null[0] == [0] * 3 and zeroed[0] == [0] * 3
            for name, a, b in zip(NAMES, null[1], zeroed[1]):
                assert float((a - b).abs().max()) <= 4 * unit(dtype) * float(t[name].abs().max()), name
        for null in (("gx",), ("gL", "gfz"), ("gx", "gZ", "glen", "gamp", "gL", "gfz")):
            part = run(lib, dtype, ar, ops, N, M, d, K, null=null)
            assert full[0] == [0] * 3 and part[0] == [0] * 3
            for name, a, b in zip(NAMES, full[1], part[1]):
                assert untouched(b) if name in null else same_bits(a, b), name
        ar.check_guards()


def test_rejected_arguments_write_nothing(lib):
    N, M, d, K = 17, 17, 3, 5
    ins = case_inputs(N, M, d, K)
    assert [lib.raw("zs_gp_max_inducing", b) for b in (4, 8, 2)] == [128, 64, 0] and lib.raw("zs_gp_max_input_dim") == 64
    for dtype in (F32, F64):
        ar = Arena(0)
        ops = [ar.put(a, dtype) for a in ins]
        outs = []
        cap = lib.raw("zs_gp_max_inducing", 4 if dtype == F32 else 8)
        for MM, dd, want in ((cap + 1, d, [ENOTSUP] * 3), (M, 65, [0, ENOTSUP, ENOTSUP]), (0, d, [EINVAL] * 3)):
            rcs, o = run(lib, dtype, ar, ops, N, MM, dd, K)
            assert rcs == want
            outs += o
        rcs, o = run(lib, dtype, ar, [None] + ops[1:], N, M, d, K)          # a NULL operand (the prepare does not take x)
        assert rcs == [0, EINVAL, EINVAL]
        outs += o
        for shares in (0, 2):          # N = 17 is one block
            rcs, o = run(lib, dtype, ar, ops, N, M, d, K, shares)
            assert rcs == [0, 0, EINVAL]
            outs += o[2:]
        torch.cuda.synchronize()
        assert all(untouched(o) for o in outs), "a rejected call wrote something"
        ar.check_guards()
    assert [lib.raw("zs_gp_row_shares", n) for n in (0, 1, 64, 65, 150, 102400)] == [0, 1, 1, 2, 3, 128]
