"""The categorical kernels through the raw C ABI of libzs_cat.so (include/zs_cat.h), on the GPU.  See tests/README_cat.md.

Truth: tests/cat_host.py ``reference_*`` -- the header's formulas in float64 -- on the same inputs (the float64 runs take the
float32 inputs widened, so one truth serves both).  Every case runs with aligned operands (the 16-byte path where N allows it)
and with every operand shifted by one element (the element path): the two must agree bit for bit, and sentinel elements around
every output must survive.  The same call twice must give the same bits."""
import math

import numpy as np
import pytest
import torch

import cat_host
from kernel_abi import DEV, EINVAL, ENOTSUP, F32, F64, I64, Arena, load, load_main, ptr, same_bits, sfx, stream

pytestmark = pytest.mark.gpu

NS = [1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 257, 1000, 4099]
RS = [1, 3, 65]
KS = [1, 2, 5]
SCALES = [0.0, 1.0, 5.0]
TAUS = [0.1, 0.5, 1.0, 5.0]
# numpy seed of a case: 1000 N + 10 R + K + SEED_SHIFT.get((N, R, K, scale), 0); the shifts keep the draws that the float64
# truth cannot decide (top-two gap of v within 1e-4 (1 + |top|)) at or below 2 % of every case (checked on the CPU)
SEED_SHIFT = {(127, 3, 5, 0.0): 100000, (1000, 3, 5, 1.0): 100000}


# ------------------------------------------------------------------------------------------------ inputs (CPU, float64)
def case_inputs(N, R, K, scale, neg_inf=True):
    """logits [R, N] (float32-representable float64; row 0 offset by +80 and row 1 by -80 when R >= 3, one -inf in the last row
    when N > 1), u [K, R, N] with 23-bit mantissas, cotangents."""
    rng = np.random.default_rng(1000 * N + 10 * R + K + SEED_SHIFT.get((N, R, K, scale), 0))
    lg = scale * rng.standard_normal((R, N))
    if R >= 3:
        lg[0] += 80.0
        lg[1] -= 80.0
    lg = lg.astype(np.float32).astype(np.float64)
    if neg_inf and N > 1:
        lg[R - 1, N // 2] = -np.inf
    u = (rng.integers(0, 1 << 23, size=(K, R, N)).astype(np.float64) + 0.5) * 2.0 ** -23
    w = rng.random((K, R, N)) * (rng.random((K, R, N)) < 0.5)
    w = w.astype(np.float32).astype(np.float64)
    if neg_inf and N > 1:
        w[:, R - 1, N // 2] = 0.0
    g = rng.standard_normal((K, R)).astype(np.float32).astype(np.float64)
    gy = rng.standard_normal((K, R, N)).astype(np.float32).astype(np.float64)
    gey = rng.standard_normal((K, R, N)).astype(np.float32).astype(np.float64)
    t = torch.from_numpy
    return dict(logits=t(lg), u=t(u), w=t(w), g=t(g), gy=t(gy), gey=t(gey))


def undecided(logits, u):
    """mask [K, R] of the draws whose float64 top-two gap of v is within 1e-4 (1 + |top|) -- about 500 x the float32 rounding
    of v -- and the float64 draw."""
    idx, lp, v = cat_host.reference_sample(logits, u)
    if v.shape[-1] == 1:
        return torch.zeros(idx.shape, dtype=torch.bool), idx, lp
    top2 = torch.topk(v, 2, dim=-1).values
    gap = top2[..., 0] - top2[..., 1]
    return ~(gap > 1e-4 * (1 + top2[..., 0].abs())), idx, lp


# ------------------------------------------------------------------------------------------------ device plumbing
@pytest.fixture(scope="module")
def lib():
    return load("cat")


@pytest.fixture(scope="module")
def main_lib():
    return load_main()


def assert_close(name, got, truth, tol):
    """|got - truth| <= tol where the truth is finite; the same infinity / a NaN where it is not."""
    got, truth = got.cpu().to(F64), truth.to(F64)
    fin = torch.isfinite(truth)
    err = (got - truth).abs()
    tol = torch.as_tensor(tol, dtype=F64).expand_as(truth)
    bad = fin & ~(err <= tol)
    ratio = torch.where(fin, err / tol.clamp(min=1e-300), torch.zeros_like(err))
    print("%s: worst error / tolerance = %.3f" % (name, float(ratio.max()) if ratio.numel() else 0.0))
    assert not bool(bad.any()), "%s: %d elements out of tolerance, worst error %.3e, worst error / tolerance %.3f" % (
        name, int(bad.sum()), float(err[bad].max()), float(ratio.max()))
    nf = ~fin
    if bool(nf.any()):
        g, t = got[nf], truth[nf]
        assert bool(((torch.isnan(g) & torch.isnan(t)) | (g == t)).all()), "%s: non-finite values differ" % name


def eps_sum(dtype, n):
    """(2^-20 + n 2^-24) for _f32, (2^-48 + n 2^-53) for _f64: the project's bound for n summed terms (README_hmc.md)."""
    return (2.0 ** -20 + n * 2.0 ** -24) if dtype == F32 else (2.0 ** -48 + n * 2.0 ** -53)


def eps_elem(dtype):
    return 2.0 ** -20 if dtype == F32 else 2.0 ** -48


def finite_abs(t):
    return torch.where(torch.isfinite(t), t.abs(), torch.zeros_like(t))


# ------------------------------------------------------------------------------------------------ raw calls
def c1(lib, dtype, ar, logits, u, K, R, N, want=(True, True, True), seed=0, call=0, rs=None):
    idx = ar.out(K * R, I64) if want[0] else None
    oh = ar.out(K * R * N, dtype) if want[1] else None
    lp = ar.out(K * R, dtype) if want[2] else None
    rc = lib.raw("zs_cat_sample_logprob" + sfx(dtype), ptr(logits), ptr(u), ptr(idx), ptr(oh), ptr(lp), K, R, N, seed, call,
                 ptr(rs), stream())
    return rc, idx, oh, lp


def c2(lib, dtype, ar, logits, idx, x, K, R, N):
    lp = ar.out(K * R, dtype)
    v = idx if x is None else x
    rc = lib.raw("zs_cat_logprob" + sfx(dtype), ptr(logits), ptr(idx), ptr(x), v.numel(), ptr(lp), K, R, N, stream())
    return rc, lp


def c2b(lib, dtype, ar, logits, idx, x, g, K, R, N, want_gx):
    gl = ar.out(R * N, dtype)
    gx = ar.out(K * R * N, dtype) if want_gx else None
    v = idx if x is None else x
    rc = lib.raw("zs_cat_logprob_bwd" + sfx(dtype), ptr(logits), ptr(idx), ptr(x), v.numel(), ptr(g), ptr(gl), ptr(gx), K, R, N,
                 stream())
    return rc, gl, gx


def c3(lib, dtype, ar, logits, u, tau, exp_space, K, R, N, seed=0, call=0, rs=None):
    y = ar.out(K * R * N, dtype)
    ey = ar.out(K * R * N, dtype) if exp_space else None
    lp = ar.out(K * R, dtype)
    rc = lib.raw("zs_cat_expconcrete_sample_logprob" + sfx(dtype), ptr(logits), ptr(u), tau, exp_space, ptr(y), ptr(ey), ptr(lp),
                 K, R, N, seed, call, ptr(rs), stream())
    return rc, y, ey, lp


def c3b(lib, dtype, ar, logits, y, tau, exp_space, gy, gey, glp, K, R, N):
    gl = ar.out(R * N, dtype)
    rc = lib.raw("zs_cat_expconcrete_sample_logprob_bwd" + sfx(dtype), ptr(logits), ptr(y), tau, exp_space, ptr(gy), ptr(gey),
                 ptr(glp), ptr(gl), K, R, N, stream())
    return rc, gl


def c4(lib, dtype, ar, logits, y, tau, exp_space, K, R, N):
    lp = ar.out(K * R, dtype)
    rc = lib.raw("zs_cat_expconcrete_logprob" + sfx(dtype), ptr(logits), ptr(y), y.numel(), tau, exp_space, ptr(lp), K, R, N,
                 stream())
    return rc, lp


def c4b(lib, dtype, ar, logits, y, tau, exp_space, glp, K, R, N):
    gy = ar.out(K * R * N, dtype)
    gl = ar.out(R * N, dtype)
    rc = lib.raw("zs_cat_expconcrete_logprob_bwd" + sfx(dtype), ptr(logits), ptr(y), y.numel(), tau, exp_space, ptr(glp), ptr(gy),
                 ptr(gl), K, R, N, stream())
    return rc, gy, gl


def grid(N):
    return [(R, K) for R in RS for K in KS] + ([(4097, 1)] if N == 3 else [])


# ------------------------------------------------------------------------------------------------ C1 and C2, forward
def logmass_tol(dtype, N, logits, idx=None, w=None):
    """(2^-20 + N 2^-24) (1 + |x l| terms + |sx lse|)"""
    lse = torch.logsumexp(logits, dim=1)[None]
    if w is None:
        picked = torch.gather(logits[None].expand(idx.shape[0], -1, -1), 2, idx.clamp(0, N - 1)[..., None])[..., 0]
        s = finite_abs(picked) + finite_abs(lse)
    else:
        s = finite_abs(torch.where(w == 0, torch.zeros_like(w), w * logits[None])).sum(-1) + finite_abs(w.sum(-1) * lse)
    return eps_sum(dtype, N) * (1 + s)


def check_draw_and_log_mass(lib, N, R, K, scale, dtypes=(F32, F64), shifts=(0, 1), d=None):
    """C1 and C2 on one shape (inputs `d`, by default case_inputs(N, R, K, scale)); returns {dtype: (idx, onehot, lp, lp at the
    index, lp of the weights, lp of the one-hot)} (CPU) of the first layout in `shifts`."""
    d = case_inputs(N, R, K, scale) if d is None else d
    lg, u, w = d["logits"], d["u"], d["w"]
    skip, tidx, tlp = undecided(lg, u)
    assert float(skip.double().mean()) <= 0.02, (N, R, K, scale, float(skip.double().mean()))
    tw = cat_host.reference_logprob_weights(lg, w)
    found = {}
    for dtype in dtypes:
        res = []
        for shift in shifts:
            ar = Arena(shift)
            dl, du, dw = ar.put(lg, dtype), ar.put(u, dtype), ar.put(w, dtype)
            rc, idx, oh, lp = c1(lib, dtype, ar, dl, du, K, R, N)
            assert rc == 0
            rc, idx_b, oh_b, lp_b = c1(lib, dtype, ar, dl, du, K, R, N)          # the same call again
            rc2, lp2 = c2(lib, dtype, ar, dl, idx, None, K, R, N)
            rc3, lpw = c2(lib, dtype, ar, dl, None, dw, K, R, N)
            rc4, lpoh = c2(lib, dtype, ar, dl, None, oh, K, R, N)
            assert rc == 0 and rc2 == 0 and rc3 == 0 and rc4 == 0
            ar.check_guards()
            assert same_bits(idx, idx_b) and same_bits(oh, oh_b) and same_bits(lp, lp_b)
            res.append((idx.cpu(), oh.cpu(), lp.cpu(), lp2.cpu(), lpw.cpu(), lpoh.cpu()))
        for a, b in zip(res[0], res[-1]):
            assert same_bits(a, b), "the aligned and the shifted layout differ (N=%d R=%d K=%d)" % (N, R, K)
        found[dtype] = res[0]
        idx, oh, lp, lp2, lpw, lpoh = res[0]
        idx = idx.view(K, R)
        assert bool(((idx >= 0) & (idx < N)).all())
        assert torch.equal(idx[~skip], tidx[~skip]), "a draw outside the margin differs from the float64 argmax"
        assert torch.equal(oh.view(K, R, N), torch.nn.functional.one_hot(idx, N).to(dtype)), "onehot is not the indicator"
        assert same_bits(lp, lp2), "C1's lp is not C2's at the drawn index"
        if N > 1:
            assert not bool((lg[torch.arange(R)[None].expand(K, R), idx] == -math.inf).any()), "a -inf category was drawn"
        else:
            assert bool((idx == 0).all()) and bool((lp == 0).all())
        own = cat_host.reference_logprob_index(lg, idx)
        assert_close("C1 lp", lp.view(K, R), own, logmass_tol(dtype, N, lg, idx=idx))
        assert_close("C2 weights", lpw.view(K, R), tw, logmass_tol(dtype, N, lg, w=w))
        # the one-hot value through the weights form: the same number as the index form, to the same bound
        assert_close("C2 one-hot", lpoh.view(K, R), own, logmass_tol(dtype, N, lg, idx=idx))
    return found


@pytest.mark.parametrize("N", NS)
def test_draw_and_log_mass(lib, N):
    for R, K in grid(N):
        for scale in SCALES:
            check_draw_and_log_mass(lib, N, R, K, scale)


def test_value_without_the_particle_axis_is_shared(lib):
    """A value of period R (R N) gives, in every entry point that takes a period, the bits of the value expanded to [K, R]."""
    N, R, K, tau = 33, 3, 5, 0.5
    d = case_inputs(N, R, K, 1.0, neg_inf=False)
    y1 = cat_host.reference_relaxed_y(d["logits"], d["u"], tau)[0]
    for dtype in (F32, F64):
        for shift in (0, 1):
            ar = Arena(shift)
            dl, dg = ar.put(d["logits"], dtype), ar.put(d["g"], dtype)
            idx1 = torch.tensor([0, 5, 32])
            w1 = d["w"][0]
            pairs = []
            for one, full in ((ar.put(idx1), ar.put(idx1[None].expand(K, R).contiguous())),):
                pairs.append((c2(lib, dtype, ar, dl, one, None, K, R, N), c2(lib, dtype, ar, dl, full, None, K, R, N)))
                pairs.append((c2b(lib, dtype, ar, dl, one, None, dg, K, R, N, False), c2b(lib, dtype, ar, dl, full, None, dg, K, R, N, False)))
            one, full = ar.put(w1, dtype), ar.put(w1[None].expand(K, R, N).contiguous(), dtype)
            pairs.append((c2(lib, dtype, ar, dl, None, one, K, R, N), c2(lib, dtype, ar, dl, None, full, K, R, N)))
            pairs.append((c2b(lib, dtype, ar, dl, None, one, dg, K, R, N, True), c2b(lib, dtype, ar, dl, None, full, dg, K, R, N, True)))
            one, full = ar.put(y1, dtype), ar.put(y1[None].expand(K, R, N).contiguous(), dtype)
            for e in (0, 1):
                pairs.append((c4(lib, dtype, ar, dl, one, tau, e, K, R, N), c4(lib, dtype, ar, dl, full, tau, e, K, R, N)))
                pairs.append((c4b(lib, dtype, ar, dl, one, tau, e, dg, K, R, N), c4b(lib, dtype, ar, dl, full, tau, e, dg, K, R, N)))
            ar.check_guards()
            for got, want in pairs:
                assert got[0] == 0 and want[0] == 0
                for x, z in zip(got[1:], want[1:]):
                    assert same_bits(x, z), "a shared value differs from the expanded one"


@pytest.mark.parametrize("N", [1, 5, 64, 257])
def test_drawn_noise_is_the_main_librarys_uniform_stream(lib, main_lib, N):
    R, K = 65, 5
    lg = case_inputs(N, R, K, 1.0)["logits"]
    n = K * R * N
    for dtype in (F32, F64):
        for seed, call, state in ((11, 3, None), (0, 2, (77, 1 << 33))):
            rs = None if state is None else torch.tensor(state, dtype=I64, device=DEV)
            noise = torch.empty(n, dtype=F32, device=DEV)
            main_lib.call("zs_philox_uniform_f32", noise.data_ptr(), n, seed, call, ptr(rs), stream())
            for shift in (0, 1):
                ar = Arena(shift)
                dl, du = ar.put(lg, dtype), ar.put(noise.cpu(), dtype)
                drawn = c1(lib, dtype, ar, dl, None, K, R, N, seed=seed, call=call, rs=rs)
                given = c1(lib, dtype, ar, dl, du, K, R, N)
                rdrawn = c3(lib, dtype, ar, dl, None, 0.5, 1, K, R, N, seed=seed, call=call, rs=rs)
                rgiven = c3(lib, dtype, ar, dl, du, 0.5, 1, K, R, N)
                ar.check_guards()
                for a, b in list(zip(drawn, given)) + list(zip(rdrawn, rgiven)):
                    if isinstance(a, int):
                        assert a == 0 and b == 0
                    else:
                        assert same_bits(a, b), "the in-kernel draw is not the injected Philox stream (N=%d)" % N


# ------------------------------------------------------------------------------------------------ C3 and C4, forward
def relaxed_tols(dtype, N, lg, u, tau, y, exp_space):
    """y: 2^-20 (1 + max_j |a_j| + |lse a|); lp: (2^-20 + N 2^-24) (1 + sum |t_j| + N |lse t| + |lgamma N|); in exp space the
    density is lp(y) - sum_j y_j, and the y_j are terms of that sum like the others: + sum |y_j|.  (Without them the bound cannot
    be met in float32 where tau < 1 makes |y_j| = |t_j - l_j| / tau the largest terms: at tau = 0.1 the kernel is at 1.28 x (N = 2)
    and 1.50 x (N = 3) of the bound without |y_j|, and so is the same formula evaluated with torch in float32: 1.30 x, 1.50 x.)"""
    a = cat_host.reference_perturbed(lg, u) / tau
    lse_a = torch.logsumexp(a, dim=-1)
    ytol = eps_elem(dtype) * (1 + finite_abs(a).max(dim=-1).values + finite_abs(lse_a))
    t = lg[None] - tau * y
    s = finite_abs(t).sum(-1) + N * finite_abs(torch.logsumexp(t, dim=-1)) + abs(math.lgamma(N))
    if exp_space:
        s = s + finite_abs(y).sum(-1)
    return ytol, eps_sum(dtype, N) * (1 + s)


def check_relaxed_draw_and_density(lib, N, R, K, scale, tau, exp_space, dtypes=(F32, F64), shifts=(0, 1), d=None):
    """C3 and C4 on one shape; returns {dtype: (y, exp(y) or None, lp, C4's lp at that y)} (CPU) of the first layout in `shifts`."""
    d = case_inputs(N, R, K, scale) if d is None else d
    lg, u = d["logits"], d["u"]
    ty, tlp = cat_host.reference_relaxed(lg, u, tau, exp_space)
    found = {}
    for dtype in dtypes:
        res = []
        for shift in shifts:
            ar = Arena(shift)
            dl, du = ar.put(lg, dtype), ar.put(u, dtype)
            rc, y, ey, lp = c3(lib, dtype, ar, dl, du, tau, exp_space, K, R, N)
            rc1, y_b, ey_b, lp_b = c3(lib, dtype, ar, dl, du, tau, exp_space, K, R, N)
            rc2, lp4 = c4(lib, dtype, ar, dl, y, tau, exp_space, K, R, N)
            assert rc == 0 and rc1 == 0 and rc2 == 0
            ar.check_guards()
            assert same_bits(y, y_b) and same_bits(ey, ey_b) and same_bits(lp, lp_b)
            res.append((y.cpu(), None if ey is None else ey.cpu(), lp.cpu(), lp4.cpu()))
        for a, b in zip(res[0], res[-1]):
            assert same_bits(a, b), "the aligned and the shifted layout differ (N=%d R=%d K=%d)" % (N, R, K)
        found[dtype] = res[0]
        y, ey, lp, lp4 = res[0]
        y = y.view(K, R, N)
        ytol, lptol = relaxed_tols(dtype, N, lg, u, tau, ty, exp_space)
        assert_close("C3 y", y, ty, ytol[..., None].expand_as(ty))
        lse_y = torch.logsumexp(y.to(F64), dim=-1)
        ok = torch.isfinite(lse_y)
        assert bool((lse_y[ok].abs() <= ytol[ok]).all()), "y is not normalised"
        assert_close("C3 lp %s" % ((N, R, K, scale, tau, exp_space),), lp.view(K, R), tlp, lptol)
        # C4 at the device's own y: the truth at that y, to the bound at that y
        t4 = cat_host.reference_relaxed_logprob(lg, y, tau, exp_space)
        _, lptol4 = relaxed_tols(dtype, N, lg, u, tau, y.to(F64), exp_space)
        assert_close("C4 lp", lp4.view(K, R), t4, lptol4)
        if exp_space:
            # exp(y) is the exp of the stored y by the kernels' own device function (zs_cat_exp runs it element-wise)
            ar = Arena(0)
            dy = ar.put(y)
            out = ar.out(y.numel(), dtype)
            assert lib.raw("zs_cat_exp" + sfx(dtype), ptr(dy), ptr(out), y.numel(), stream()) == 0
            ar.check_guards()
            assert same_bits(out, ey), "exp(y) is not the device exp of the y written"
    return found


@pytest.mark.parametrize("N", NS)
def test_relaxed_draw_and_density(lib, N):
    for R, K in grid(N):
        for ci, scale in enumerate(SCALES):
            tau = TAUS[(ci + KS.index(K) + RS.index(R if R in RS else 1)) % 4]
            exp_space = (ci + K) % 2
            check_relaxed_draw_and_density(lib, N, R, K, scale, tau, exp_space)


# ------------------------------------------------------------------------------------------------ backward
def bwd_tol(dtype, N, K):
    """(2^-20 + (N + K) 2^-24) for _f32, (2^-48 + (N + K) 2^-53) for _f64: times the sum of the magnitudes of the terms added"""
    return (2.0 ** -20 + (N + K) * 2.0 ** -24) if dtype == F32 else (2.0 ** -48 + (N + K) * 2.0 ** -53)


def exponent_eps(dtype):
    """A softmax factor exp(a - b) is the exponential of a difference of two ROUNDED numbers: a and the difference are rounded
    once each, b (a logsumexp) at least once, so the exponent is off by up to 2 * 2^-24 (|a| + |b|) and the factor by that much
    relatively.  This enters a bound additively, as exponent_eps * (|a| + |b|) * |the term that carries the factor|: nothing
    for rows of small logits, the dominant part on the rows offset by +-80."""
    return 2.0 * (2.0 ** -24 if dtype == F32 else 2.0 ** -53)


def check_log_mass_backward(lib, N, R, K, scale, dtypes=(F32, F64), shifts=(0, 1), d=None):
    """C2's backward on one shape (inputs without a -inf logit); returns {dtype: (glogits of the index form, glogits and gx of the
    weights form)} (CPU) of the first layout in `shifts`."""
    d = case_inputs(N, R, K, scale, neg_inf=False) if d is None else d
    lg, w, g, u = d["logits"], d["w"], d["g"], d["u"]
    idx = cat_host.reference_sample(lg, u)[0]
    sm = torch.softmax(lg, dim=1)
    lse = torch.logsumexp(lg, dim=1)
    truths = {}
    for form, x in (("index", torch.nn.functional.one_hot(idx, N).to(F64)), ("weights", w)):
        l0 = lg.clone().requires_grad_(True)
        x0 = x.clone().requires_grad_(True)
        lp = (x0 * l0[None]).sum(-1) - x0.sum(-1) * torch.logsumexp(l0, dim=1)[None]
        gl, gx = torch.autograd.grad(lp, [l0, x0], g)
        # terms of glogits: |g x| and |g sx softmax| over k; the softmax is exp(l - lse)
        soft = ((g.abs() * x.sum(-1).abs()).sum(0))[:, None] * sm
        s_gl = (g.abs()[..., None] * x.abs()).sum(0) + soft
        x_gl = soft * (lg.abs() + lse.abs()[:, None])
        s_gx = g.abs()[..., None] * (lg.abs() + lse.abs()[:, None])[None]
        truths[form] = (x, gl, gx, s_gl, x_gl, s_gx)
    found = {}
    for dtype in dtypes:
        res = []
        for shift in shifts:
            ar = Arena(shift)
            dl, dg = ar.put(lg, dtype), ar.put(g, dtype)
            didx = ar.put(idx)
            rc, gl_i, _ = c2b(lib, dtype, ar, dl, didx, None, dg, K, R, N, False)
            rc1, gl_i2, _ = c2b(lib, dtype, ar, dl, didx, None, dg, K, R, N, False)
            dw = ar.put(w, dtype)
            rc2, gl_w, gx_w = c2b(lib, dtype, ar, dl, None, dw, dg, K, R, N, True)
            rc3, gl_w2, gx_w2 = c2b(lib, dtype, ar, dl, None, dw, dg, K, R, N, True)
            assert rc == 0 and rc1 == 0 and rc2 == 0 and rc3 == 0
            ar.check_guards()
            assert same_bits(gl_i, gl_i2) and same_bits(gl_w, gl_w2) and same_bits(gx_w, gx_w2), \
                "K-summed gradients differ between two calls"
            res.append((gl_i.cpu(), gl_w.cpu(), gx_w.cpu()))
        for a, b in zip(res[0], res[-1]):
            assert same_bits(a, b), "the aligned and the shifted layout differ (N=%d R=%d K=%d)" % (N, R, K)
        found[dtype] = res[0]
        gl_i, gl_w, gx_w = res[0]
        e, ee = bwd_tol(dtype, N, K), exponent_eps(dtype)
        for form, got in (("index", gl_i), ("weights", gl_w)):
            x, gl, gx, s_gl, x_gl, s_gx = truths[form]
            assert_close("glogits (%s)" % form, got.view(R, N), gl, e * s_gl + ee * x_gl + 1e-300)
        assert_close("gx", gx_w.view(K, R, N), truths["weights"][2], e * truths["weights"][5] + 1e-300)
    return found


@pytest.mark.parametrize("N", NS)
def test_log_mass_backward(lib, N):
    for R, K in grid(N):
        for scale in SCALES:
            check_log_mass_backward(lib, N, R, K, scale)


def check_relaxed_backward(lib, N, R, K, scale, tau, exp_space, dtypes=(F32, F64), shifts=(0, 1), d=None):
    """The backwards of C3 and C4 on one shape (inputs without a -inf logit); returns {dtype: (y, C3's glogits, C4's gy, C4's
    glogits)} (CPU) of the first layout in `shifts`."""
    d = case_inputs(N, R, K, scale, neg_inf=False) if d is None else d
    lg, u, g, gy, gey = d["logits"], d["u"], d["g"], d["gy"], d["gey"]
    found = {}
    for dtype in dtypes:
        res = []
        for shift in shifts:
            ar = Arena(shift)
            dl, du = ar.put(lg, dtype), ar.put(u, dtype)
            rc, y, ey, lp = c3(lib, dtype, ar, dl, du, tau, exp_space, K, R, N)
            dgy, dgey, dg = ar.put(gy, dtype), (ar.put(gey, dtype) if exp_space else None), ar.put(g, dtype)
            rc1, gl3 = c3b(lib, dtype, ar, dl, y, tau, exp_space, dgy, dgey, dg, K, R, N)
            rc2, gl3_b = c3b(lib, dtype, ar, dl, y, tau, exp_space, dgy, dgey, dg, K, R, N)
            rc3, gy4, gl4 = c4b(lib, dtype, ar, dl, y, tau, exp_space, dg, K, R, N)
            rc4, gy4_b, gl4_b = c4b(lib, dtype, ar, dl, y, tau, exp_space, dg, K, R, N)
            assert rc == 0 and rc1 == 0 and rc2 == 0 and rc3 == 0 and rc4 == 0
            ar.check_guards()
            assert same_bits(gl3, gl3_b) and same_bits(gl4, gl4_b) and same_bits(gy4, gy4_b), \
                "K-summed gradients differ between two calls"
            res.append((y.cpu(), gl3.cpu(), gy4.cpu(), gl4.cpu()))
        for a, b in zip(res[0], res[-1]):
            assert same_bits(a, b), "the aligned and the shifted layout differ (N=%d R=%d K=%d)" % (N, R, K)
        found[dtype] = res[0]
        ys, gl3, gy4, gl4 = res[0]
        ys = ys.view(K, R, N).to(F64)
        # float64 autograd of the restatement at the noise that reproduces the saved y: gumbel = tau y_saved - logits
        gum = tau * ys - lg[None]
        l0 = lg.clone().requires_grad_(True)
        a = (l0[None] + gum) / tau
        yv = a - torch.logsumexp(a, dim=-1, keepdim=True)
        lpv = cat_host.reference_relaxed_logprob(l0, yv, tau, exp_space)
        out = (gy * yv).sum() + (g * lpv).sum() + ((gey * torch.exp(yv)).sum() if exp_space else 0.0)
        t3, = torch.autograd.grad(out, [l0])
        y1 = ys.clone().requires_grad_(True)
        l1 = lg.clone().requires_grad_(True)
        t4y, t4l = torch.autograd.grad(cat_host.reference_relaxed_logprob(l1, y1, tau, exp_space), [y1, l1], g)
        # magnitudes of the terms added (header formulas); q = 1 - N softmax(t) carries the softmax exp(t - lse t)
        e_ = 1.0 if exp_space else 0.0
        ga = g.abs()[..., None]
        t = lg[None] - tau * ys
        lse_t = torch.logsumexp(t, dim=-1, keepdim=True)
        nsm = N * torch.softmax(t, dim=-1)
        qa = 1 + nsm
        dq = nsm * (t.abs() + lse_t.abs())          # times exponent_eps: the rounding of q
        ex = torch.exp(ys)
        G = gy.abs() + (gey.abs() * ex if exp_space else 0.0) + ga * (tau * qa + e_)
        s3 = ((G + ex * G.sum(-1, keepdim=True)) / tau + ga * qa).sum(0)
        # q enters G (times tau, over tau) and the direct term; exp(y) stands for softmax(a) = exp(a - lse a), whose
        # exponent the stored y carries rounded
        aa = cat_host.reference_perturbed(lg, u) / tau
        da = ex * (aa.abs() + torch.logsumexp(aa, dim=-1, keepdim=True).abs())
        x3 = (2 * ga * dq + da * G.sum(-1, keepdim=True) / tau).sum(0)
        s4y, x4y = ga * (tau * qa + e_), ga * tau * dq
        s4l, x4l = (ga * qa).sum(0), (ga * dq).sum(0)
        e, ee = bwd_tol(dtype, N, K), exponent_eps(dtype)
        assert_close("C3 glogits %s" % ((N, R, K, scale, tau, exp_space),), gl3.view(R, N), t3, e * s3 + ee * x3)
        assert_close("C4 gy", gy4.view(K, R, N), t4y, e * s4y + ee * x4y)
        assert_close("C4 glogits", gl4.view(R, N), t4l, e * s4l + ee * x4l)
    return found


@pytest.mark.parametrize("N", NS)
def test_relaxed_backward(lib, N):
    for R, K in grid(N):
        ci = RS.index(R if R in RS else 1) + KS.index(K)
        for si, scale in enumerate(SCALES):
            tau = TAUS[(ci + si) % 4]
            exp_space = (ci + si) % 2
            check_relaxed_backward(lib, N, R, K, scale, tau, exp_space)


# ------------------------------------------------------------------------------------------------ guards and rejections
def test_out_of_range_index_gives_nan_for_that_draw_only(lib):
    N, R, K = 33, 65, 2
    d = case_inputs(N, R, K, 1.0, neg_inf=False)
    idx = cat_host.reference_sample(d["logits"], d["u"])[0]
    for dtype in (F32, F64):
        ar = Arena(0)
        dl = ar.put(d["logits"], dtype)
        rc, good = c2(lib, dtype, ar, dl, ar.put(idx), None, K, R, N)
        bad_idx = idx.clone()
        spots = [(0, 0), (1, 17), (1, 64)]
        for (k, r), v in zip(spots, (-1, N, 1 << 40)):
            bad_idx[k, r] = v
        rc2, bad = c2(lib, dtype, ar, dl, ar.put(bad_idx), None, K, R, N)
        assert rc == 0 and rc2 == 0
        ar.check_guards()
        good, bad = good.cpu().view(K, R), bad.cpu().view(K, R)
        mask = torch.zeros(K, R, dtype=torch.bool)
        for k, r in spots:
            mask[k, r] = True
        assert bool(torch.isnan(bad[mask]).all())
        assert same_bits(good[~mask], bad[~mask])


def test_rejected_arguments_write_nothing(lib):
    N, R, K = 5, 3, 2
    d = case_inputs(N, R, K, 1.0)
    for dtype in (F32, F64):
        ar = Arena(0)
        dl, du, dg = ar.put(d["logits"], dtype), ar.put(d["u"], dtype), ar.put(d["g"], dtype)
        didx = ar.put(torch.zeros(K, R, dtype=I64))
        # every output any entry point could write, of the full size of the valid problem
        oi, on, on2, ol, og = ar.out(K * R, I64), ar.out(K * R * N, dtype), ar.out(K * R * N, dtype), ar.out(K * R, dtype), ar.out(R * N, dtype)
        s, st = sfx(dtype), stream()
        p = ptr

        def every(lgp, k, r, n, tau, relaxed_only=False):
            """the return codes of all entry points (or of the four with a temperature) on these arguments"""
            return ([] if relaxed_only else [
                lib.raw("zs_cat_sample_logprob" + s, p(lgp), p(du), p(oi), p(on), p(ol), k, r, n, 0, 0, None, st),
                lib.raw("zs_cat_logprob" + s, p(lgp), p(didx), None, K * R, p(ol), k, r, n, st),
                lib.raw("zs_cat_logprob_bwd" + s, p(lgp), None, p(du), K * R * N, p(dg), p(og), p(on), k, r, n, st)]) + [
                lib.raw("zs_cat_expconcrete_sample_logprob" + s, p(lgp), p(du), tau, 1, p(on), p(on2), p(ol), k, r, n, 0, 0, None, st),
                lib.raw("zs_cat_expconcrete_sample_logprob_bwd" + s, p(lgp), p(du), tau, 0, p(du), None, p(dg), p(og), k, r, n, st),
                lib.raw("zs_cat_expconcrete_logprob" + s, p(lgp), p(du), K * R * N, tau, 0, p(ol), k, r, n, st),
                lib.raw("zs_cat_expconcrete_logprob_bwd" + s, p(lgp), p(du), K * R * N, tau, 0, p(dg), p(on), p(og), k, r, n, st)]

        assert every(None, K, R, N, 0.5) == [EINVAL] * 7
        for k, r, n in ((K, R, 0), (K, R, -3), (-1, R, N), (K, -1, N)):
            assert every(dl, k, r, n, 0.5) == [EINVAL] * 7
        for tau in (0.0, -1.0, float("nan"), float("inf")):
            assert every(dl, K, R, N, tau, relaxed_only=True) == [EINVAL] * 4
        assert every(dl, K, R, 1 << 31, 0.5) == [ENOTSUP] * 7
        assert every(dl, 0, R, N, 0.5) == [0] * 7 and every(dl, K, 0, N, 0.5) == [0] * 7          # K R == 0 launches nothing
        assert lib.raw("zs_cat_logprob" + s, p(dl), p(didx), p(du), K * R, p(ol), K, R, N, st) == EINVAL          # both forms at once
        assert lib.raw("zs_cat_logprob" + s, p(dl), None, None, K * R, p(ol), K, R, N, st) == EINVAL               # no value
        assert lib.raw("zs_cat_logprob" + s, p(dl), p(didx), None, K * R + 1, p(ol), K, R, N, st) == EINVAL        # a period that is none
        assert lib.raw("zs_cat_sample_logprob" + s, p(dl), p(du), None, None, None, K, R, N, 0, 0, None, st) == EINVAL   # nothing to write
        torch.cuda.synchronize()
        assert ar.untouched(), "a rejected call wrote something"
    assert lib.raw("zs_cat_group_lanes", 0) == 0 and lib.raw("zs_cat_group_lanes", 4) == 1 and lib.raw("zs_cat_group_lanes", 4099) == 64
