"""The multivariate-normal kernels through the raw C ABI of libzs_mvn.so (include/zs_mvn.h), on the GPU.  See tests/README_mvn.md.

Truth: tests/mvn_host.py ``reference_*`` -- the header's formulas in float64 -- on the same inputs (the float64 runs take the
float32 inputs widened, so one truth serves both).  The upper triangle of every ``tril`` handed to a kernel is NaN: it is never
read.  Every case runs with aligned operands and with every operand shifted by one element: the two must agree bit for bit, and
sentinel elements around every output must survive.  The same call twice must give the same bits.

Tolerances (derived, not tuned; u = 2^-24 for _f32, 2^-53 for _f64; Higham, Accuracy and Stability, ch. 8, for the substitutions):
  e    = (D + 3) u |L^-1| (|L| |y| + |x| + |mean|)                          the error of y = L^-1 (x - mean), componentwise
  e_w  = (D + 3) u |L^-T| (|L^T| |w|) + |L^-T| e                             the error of w = L^-T y
  V2 lp    sum_i |y_i| e_i + (D + 4) u (1/2 sum y^2 + sum |log L_ii| + D/2 log 2 pi)
  V1 z     (D + 2) u (|mean| + |L| |eps|);    V1 lp  (D + 4) u (sum of the magnitudes of its terms)
  gtril    2 [sum_k |g_k| (e_w,i |y_j| + |w_i| e_j) + (K + 2) u sum_k |terms|],  gmean likewise with sum_k |g_k| e_w,i"""
import math

import numpy as np
import pytest
import torch

import mvn_host
from kernel_abi import DEV, EINVAL, ENOTSUP, F32, F64, I64, Arena, load, load_main, ptr, same_bits, sfx, stream, unit

pytestmark = pytest.mark.gpu

DS = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 32, 33, 63, 64]
RS = [1, 3, 65]
KS = [1, 2, 5]
LOG_2PI = math.log(2.0 * math.pi)
WORST = {}          # quantity -> the worst error / tolerance seen in this session (printed; recorded in README_mvn.md)


# ------------------------------------------------------------------------------------------------ inputs (CPU, float64)
def f32r(a):
    return torch.from_numpy(np.asarray(a).astype(np.float32).astype(np.float64))


def case_inputs(D, R, K):
    """float32-representable float64 operands: L with diagonal U[0.5, 2], strict lower part N(0, 1) 0.5 / sqrt(D) and a NaN upper
    triangle, mean ~ 3 N(0, 1), x = mean + 2 N(0, 1), eps ~ N(0, 1), cotangents ~ N(0, 1)."""
    rng = np.random.default_rng(1000 * D + 10 * R + K)
    L = np.tril(rng.standard_normal((R, D, D)) * 0.5 / math.sqrt(D), -1)
    L[:, np.arange(D), np.arange(D)] = rng.uniform(0.5, 2.0, (R, D))
    L[:, np.triu_indices(D, 1)[0], np.triu_indices(D, 1)[1]] = np.nan
    mean = f32r(3.0 * rng.standard_normal((R, D)))
    x = f32r(mean.numpy()[None] + 2.0 * rng.standard_normal((K, R, D)))
    return dict(tril=f32r(L), mean=mean, x=x, eps=f32r(rng.standard_normal((K, R, D))), g=f32r(rng.standard_normal((K, R))),
                gz=f32r(rng.standard_normal((K, R, D))))


def grid(D):
    return [(R, K) for R in RS for K in KS] + ([(4097, 1)] if D == 3 else [])


# ------------------------------------------------------------------------------------------------ device plumbing
@pytest.fixture(scope="module")
def lib():
    return load("mvn")


@pytest.fixture(scope="module")
def main_lib():
    return load_main()


def assert_close(name, got, truth, tol):
    got, truth = got.cpu().to(F64), truth.to(F64)
    tol = torch.as_tensor(tol, dtype=F64).expand_as(truth)
    err = (got - truth).abs()
    ratio = float((err / tol.clamp(min=1e-300)).max()) if err.numel() else 0.0
    key = name.split(" [")[0]
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print("%s: worst error / tolerance = %.3f" % (name, ratio))
    assert bool(torch.isfinite(got).all()), "%s: non-finite values" % name
    assert bool((err <= tol).all()), "%s: %d elements out of tolerance, worst error / tolerance %.3f" % (
        name, int((err > tol).sum()), ratio)


# ------------------------------------------------------------------------------------------------ raw calls
def v1(lib, dtype, ar, mean, tril, eps, K, R, D, seed=0, call=0, rs=None):
    z, lp = ar.out(K * R * D, dtype), ar.out(K * R, dtype)
    rc = lib.raw("zs_mvn_sample_logprob" + sfx(dtype), ptr(mean), ptr(tril), ptr(eps), ptr(z), ptr(lp), K, R, D, seed, call,
                 ptr(rs), stream())
    return rc, z, lp


def v1b(lib, dtype, ar, tril, eps, gz, glp, reparam, K, R, D, seed=0, call=0, rs=None):
    gm, gt = ar.out(R * D, dtype), ar.out(R * D * D, dtype)
    rc = lib.raw("zs_mvn_sample_logprob_bwd" + sfx(dtype), ptr(tril), ptr(eps), ptr(gz), ptr(glp), reparam, ptr(gm), ptr(gt),
                 K, R, D, seed, call, ptr(rs), stream())
    return rc, gm, gt


def v2(lib, dtype, ar, mean, tril, x, K, R, D):
    lp = ar.out(K * R, dtype)
    rc = lib.raw("zs_mvn_logprob" + sfx(dtype), ptr(mean), ptr(tril), ptr(x), x.numel(), ptr(lp), K, R, D, stream())
    return rc, lp


def v2b(lib, dtype, ar, mean, tril, x, glp, K, R, D):
    gx, gm, gt = ar.out(K * R * D, dtype), ar.out(R * D, dtype), ar.out(R * D * D, dtype)
    rc = lib.raw("zs_mvn_logprob_bwd" + sfx(dtype), ptr(mean), ptr(tril), ptr(x), x.numel(), ptr(glp), ptr(gx), ptr(gm),
                 ptr(gt), K, R, D, stream())
    return rc, gx, gm, gt


# ------------------------------------------------------------------------------------------------ the bounds
class Bounds(object):
    """The componentwise bounds of the module docstring for one case, in float64 on the CPU."""

    def __init__(self, dtype, mean, tril, K):
        self.u = unit(dtype)
        self.L = mvn_host.lower(tril)
        self.R, self.D = mean.shape
        self.K = K
        self.mean = mean
        self.aL = self.L.abs()
        self.aLi = torch.linalg.inv(self.L).abs()
        self.diag = torch.diagonal(self.L, dim1=-2, dim2=-1)
        self.const = 0.5 * self.D * LOG_2PI + torch.log(self.diag).abs().sum(-1)          # [R]

    def mv(self, M, v):
        return torch.einsum("rij,krj->kri", M, v)

    def e_y(self, x, y):
        return (self.D + 3) * self.u * self.mv(self.aLi, self.mv(self.aL, y.abs()) + x.abs() + self.mean.abs()[None])

    def e_w(self, w, e):
        aLiT, aLT = self.aLi.transpose(-1, -2), self.aL.transpose(-1, -2)
        return (self.D + 3) * self.u * self.mv(aLiT, self.mv(aLT, w.abs())) + self.mv(aLiT, e)

    def lp(self, y, e=None):
        t = (self.D + 4) * self.u * (0.5 * (y ** 2).sum(-1) + self.const[None])
        return t if e is None else t + (y.abs() * e).sum(-1)

    def z(self, eps):
        return (self.D + 2) * self.u * (self.mean.abs()[None] + self.mv(self.aL, eps.abs()))

    def score(self, g, w, y, e, ew):
        """(tolerance of gmean [R, D], of gtril [R, D, D]) for the k-sums of g w and g (w y^T - diag(1 / L_ii))"""
        ga = g.abs()
        ku = (self.K + 2) * self.u
        gm = 2 * ((ga[..., None] * ew).sum(0) + ku * (ga[..., None] * w.abs()).sum(0))
        terms = torch.einsum("kr,kri,krj->rij", ga, w.abs(), y.abs()) + torch.diag_embed(ga.sum(0)[:, None] / self.diag)
        gt = 2 * (torch.einsum("kr,kri,krj->rij", ga, ew, y.abs()) + torch.einsum("kr,kri,krj->rij", ga, w.abs(), e) + ku * terms)
        return gm, gt + 1e-300

    def reparam(self, gz, eps, g):
        ku = (self.K + 2) * self.u
        gm = 2 * ku * gz.abs().sum(0)
        terms = torch.einsum("kri,krj->rij", gz.abs(), eps.abs()) + torch.diag_embed(g.abs().sum(0)[:, None] / self.diag)
        return gm + 1e-300, 2 * ku * terms + 1e-300


def lower_of(gt, R, D):
    """(the lower triangle as a dense [R, D, D] with zeros above, whether the upper triangle is exactly zero)"""
    gt = gt.cpu().view(R, D, D)
    up = torch.triu(gt, 1)
    return torch.tril(gt), bool((up == 0).all()) and not bool(torch.isnan(up).any())


# ------------------------------------------------------------------------------------------------ the grid
def check_forward_and_backward(lib, D, R, K, dtypes=(F32, F64), shifts=(0, 1), d=None):
    """Every entry point on one shape (inputs `d`, by default case_inputs(D, R, K)) against the float64 truths and the derived
    bounds; returns {dtype: [z, lp1, lp2, lpz, gx, gm2, gt2, gx1, gm0, gt0, gm1, gt1]} (CPU) of the first layout in `shifts`."""
    d = case_inputs(D, R, K) if d is None else d
    mean, tril, x, eps, g, gz = d["mean"], d["tril"], d["x"], d["eps"], d["g"], d["gz"]
    ones = torch.ones_like(g)
    tz, tlp1 = mvn_host.reference_sample(mean, tril, eps)
    ty = mvn_host.reference_whiten(mean, tril, x)
    tlp2 = mvn_host.reference_density(tril, ty)
    tw, tgm2, tgt2 = mvn_host.reference_score(tril, ty, g)
    tw1, tgm1, tgt1 = mvn_host.reference_score(tril, eps, g)
    tgm0, tgt0 = mvn_host.reference_sample_bwd(tril, eps, gz, g)
    found = {}
    for dtype in dtypes:
        res = []
        for shift in shifts:
            ar = Arena(shift)
            dm, dt, dx, de = ar.put(mean, dtype), ar.put(tril, dtype), ar.put(x, dtype), ar.put(eps, dtype)
            dg, dgz, d1 = ar.put(g, dtype), ar.put(gz, dtype), ar.put(ones, dtype)
            outs, twice = [], []
            for rep in range(2):          # the same calls again: the same bits
                o = []
                rc, z, lp1 = v1(lib, dtype, ar, dm, dt, de, K, R, D)
                o += [rc, z, lp1]
                rc, lp2 = v2(lib, dtype, ar, dm, dt, dx, K, R, D)
                o += [rc, lp2]
                rc, lpz = v2(lib, dtype, ar, dm, dt, z, K, R, D)
                o += [rc, lpz]
                o += list(v2b(lib, dtype, ar, dm, dt, dx, dg, K, R, D))
                o += list(v2b(lib, dtype, ar, dm, dt, dx, d1, K, R, D))[:2]
                o += list(v1b(lib, dtype, ar, dt, de, dgz, dg, 1, K, R, D))
                o += list(v1b(lib, dtype, ar, dt, de, None, dg, 0, K, R, D))
                (outs if rep == 0 else twice).extend(o)
            ar.check_guards()
            for a, b in zip(outs, twice):
                if isinstance(a, int):
                    assert a == 0 and b == 0
                else:
                    assert same_bits(a, b), "two identical calls differ (D=%d R=%d K=%d)" % (D, R, K)
            res.append([a.cpu() for a in outs if not isinstance(a, int)])
        for a, b in zip(res[0], res[-1]):
            assert same_bits(a, b), "the aligned and the shifted layout differ (D=%d R=%d K=%d)" % (D, R, K)
        found[dtype] = res[0]
        z, lp1, lp2, lpz, gx, gm2, gt2, gx1, gm0, gt0, gm1, gt1 = res[0]
        B = Bounds(dtype, mean, tril, K)
        tag = " [D=%d R=%d K=%d %s]" % (D, R, K, sfx(dtype))
        # V1
        assert_close("V1 z" + tag, z.view(K, R, D), tz, B.z(eps))
        assert_close("V1 lp" + tag, lp1.view(K, R), tlp1, B.lp(eps))
        # V2
        e = B.e_y(x, ty)
        assert_close("V2 lp" + tag, lp2.view(K, R), tlp2, B.lp(ty, e))
        # V2 at V1's own draw against V1's lp: within the sum of the two bounds
        zd = z.view(K, R, D).to(F64)
        yz = mvn_host.reference_whiten(mean, tril, zd)
        assert_close("V2 at V1's z" + tag, lpz.view(K, R), lp1.view(K, R).to(F64), B.lp(eps) + B.lp(yz, B.e_y(zd, yz)))
        # back substitution, read back through gx with glp = 1
        ew = B.e_w(tw, e)
        assert_close("w" + tag, -gx1.view(K, R, D).to(F64), tw, ew)
        assert_close("V2 gx" + tag, gx.view(K, R, D), -g[..., None] * tw, g.abs()[..., None] * ew + B.u * (g[..., None] * tw).abs())
        # gradients
        tolm, tolt = B.score(g, tw, ty, e, ew)
        assert_close("V2 gmean" + tag, gm2.view(R, D), tgm2, tolm)
        low, zero = lower_of(gt2, R, D)
        assert zero, "gtril's upper triangle is not exactly zero"
        assert_close("V2 gtril" + tag, low, tgt2, tolt)
        ew1 = B.e_w(tw1, torch.zeros_like(eps))
        tolm, tolt = B.score(g, tw1, eps, torch.zeros_like(eps), ew1)
        assert_close("V1 gmean (detached draw)" + tag, gm1.view(R, D), tgm1, tolm)
        low, zero = lower_of(gt1, R, D)
        assert zero, "gtril's upper triangle is not exactly zero"
        assert_close("V1 gtril (detached draw)" + tag, low, tgt1, tolt)
        tolm, tolt = B.reparam(gz, eps, g)
        assert_close("V1 gmean" + tag, gm0.view(R, D), tgm0, tolm)
        low, zero = lower_of(gt0, R, D)
        assert zero, "gtril's upper triangle is not exactly zero"
        assert_close("V1 gtril" + tag, low, tgt0, tolt)
    return found


@pytest.mark.parametrize("D", DS)
def test_forward_and_backward_against_float64(lib, D):
    for R, K in grid(D):
        check_forward_and_backward(lib, D, R, K)
    print("worst error / tolerance so far: %s" % ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def test_value_without_the_particle_axis_is_shared(lib):
    """A value of period R D gives the bits of the value expanded to [K, R, D], forward and backward."""
    D, R, K = 17, 3, 5
    d = case_inputs(D, R, K)
    x1 = d["x"][0]
    for dtype in (F32, F64):
        for shift in (0, 1):
            ar = Arena(shift)
            dm, dt, dg = ar.put(d["mean"], dtype), ar.put(d["tril"], dtype), ar.put(d["g"], dtype)
            one, full = ar.put(x1, dtype), ar.put(x1[None].expand(K, R, D).contiguous(), dtype)
            pairs = [(v2(lib, dtype, ar, dm, dt, one, K, R, D), v2(lib, dtype, ar, dm, dt, full, K, R, D)),
                     (v2b(lib, dtype, ar, dm, dt, one, dg, K, R, D), v2b(lib, dtype, ar, dm, dt, full, dg, K, R, D))]
            ar.check_guards()
            for got, want in pairs:
                assert got[0] == 0 and want[0] == 0
                for a, b in zip(got[1:], want[1:]):
                    assert same_bits(a, b), "a shared value differs from the expanded one"


@pytest.mark.parametrize("D", [1, 5, 33, 64])
def test_drawn_noise_is_the_main_librarys_normal_stream(lib, main_lib, D):
    R, K = 65, 5
    d = case_inputs(D, R, K)
    n = K * R * D
    for dtype in (F32, F64):
        for seed, call, state in ((11, 3, None), (0, 2, (77, 1 << 33))):
            rs = None if state is None else torch.tensor(state, dtype=I64, device=DEV)
            noise = torch.empty(n, dtype=F32, device=DEV)
            main_lib.call("zs_philox_normal_f32", noise.data_ptr(), n, seed, call, ptr(rs), stream())
            for shift in (0, 1):
                ar = Arena(shift)
                dm, dt, de = ar.put(d["mean"], dtype), ar.put(d["tril"], dtype), ar.put(noise.cpu(), dtype)
                dg, dgz = ar.put(d["g"], dtype), ar.put(d["gz"], dtype)
                pairs = [(v1(lib, dtype, ar, dm, dt, None, K, R, D, seed=seed, call=call, rs=rs), v1(lib, dtype, ar, dm, dt, de, K, R, D))]
                for reparam in (1, 0):
                    pairs.append((v1b(lib, dtype, ar, dt, None, dgz, dg, reparam, K, R, D, seed=seed, call=call, rs=rs),
                                  v1b(lib, dtype, ar, dt, de, dgz, dg, reparam, K, R, D)))
                ar.check_guards()
                for drawn, given in pairs:
                    assert drawn[0] == 0 and given[0] == 0
                    for a, b in zip(drawn[1:], given[1:]):
                        assert same_bits(a, b), "the in-kernel draw is not the injected Philox stream (D=%d)" % D


def test_a_bad_diagonal_gives_inf_or_nan_without_a_trap(lib):
    D, R, K = 3, 3, 2
    d = case_inputs(D, R, K)
    tril = d["tril"].clone()
    tril[0, 1, 1] = 0.0
    tril[1, 2, 2] = -1.0
    for dtype in (F32, F64):
        ar = Arena(0)
        rc, z, lp = v1(lib, dtype, ar, ar.put(d["mean"], dtype), ar.put(tril, dtype), ar.put(d["eps"], dtype), K, R, D)
        ar.check_guards()
        lp = lp.cpu().view(K, R)
        assert rc == 0 and bool((lp[:, 0] == math.inf).all()) and bool(torch.isnan(lp[:, 1]).all()) and bool(torch.isfinite(lp[:, 2]).all())


def test_rejected_arguments_write_nothing(lib):
    D, R, K = 5, 3, 2
    d = case_inputs(D, R, K)
    for dtype in (F32, F64):
        ar = Arena(0)
        dm, dt, de, dg = ar.put(d["mean"], dtype), ar.put(d["tril"], dtype), ar.put(d["eps"], dtype), ar.put(d["g"], dtype)
        oz, ol, om, ot = ar.out(K * R * D, dtype), ar.out(K * R, dtype), ar.out(R * D, dtype), ar.out(R * D * D, dtype)
        s, st, p = sfx(dtype), stream(), ptr

        def every(mp, tp, k, r, n):
            return [lib.raw("zs_mvn_sample_logprob" + s, p(mp), p(tp), p(de), p(oz), p(ol), k, r, n, 0, 0, None, st),
                    lib.raw("zs_mvn_sample_logprob_bwd" + s, p(tp), p(de), p(de), p(dg), 1, p(om), p(ot), k, r, n, 0, 0, None, st),
                    lib.raw("zs_mvn_sample_logprob_bwd" + s, p(tp), p(de), None, p(dg), 0, p(om), p(ot), k, r, n, 0, 0, None, st),
                    lib.raw("zs_mvn_logprob" + s, p(mp), p(tp), p(de), K * R * D, p(ol), k, r, n, st),
                    lib.raw("zs_mvn_logprob_bwd" + s, p(mp), p(tp), p(de), K * R * D, p(dg), p(oz), p(om), p(ot), k, r, n, st)]

        assert every(dm, None, K, R, D) == [EINVAL] * 5
        # a NULL mean (the backward of V1 takes none)
        assert lib.raw("zs_mvn_sample_logprob" + s, None, p(dt), p(de), p(oz), p(ol), K, R, D, 0, 0, None, st) == EINVAL
        assert lib.raw("zs_mvn_logprob" + s, None, p(dt), p(de), K * R * D, p(ol), K, R, D, st) == EINVAL
        assert lib.raw("zs_mvn_logprob_bwd" + s, None, p(dt), p(de), K * R * D, p(dg), p(oz), p(om), p(ot), K, R, D, st) == EINVAL
        for k, r, n in ((K, R, 0), (K, R, -3), (-1, R, D), (K, -1, D)):
            assert every(dm, dt, k, r, n) == [EINVAL] * 5
        assert every(dm, dt, K, R, 65) == [ENOTSUP] * 5 and every(dm, dt, K, R, 1 << 31) == [ENOTSUP] * 5
        assert every(dm, dt, 0, R, D) == [0] * 5 and every(dm, dt, K, 0, D) == [0] * 5          # K R == 0 launches nothing
        assert lib.raw("zs_mvn_logprob" + s, p(dm), p(dt), p(de), K * R * D + 1, p(ol), K, R, D, st) == EINVAL      # a period that is none
        assert lib.raw("zs_mvn_logprob_bwd" + s, p(dm), p(dt), p(de), D, p(dg), p(oz), p(om), p(ot), K, R, D, st) == EINVAL
        assert lib.raw("zs_mvn_logprob" + s, p(dm), p(dt), None, K * R * D, p(ol), K, R, D, st) == EINVAL           # no value
        assert lib.raw("zs_mvn_sample_logprob" + s, p(dm), p(dt), p(de), None, None, K, R, D, 0, 0, None, st) == EINVAL  # nothing to write
        assert lib.raw("zs_mvn_sample_logprob_bwd" + s, p(dt), p(de), None, None, 1, p(om), p(ot), K, R, D, 0, 0, None, st) == EINVAL
        assert lib.raw("zs_mvn_sample_logprob_bwd" + s, p(dt), p(de), p(de), None, 0, p(om), p(ot), K, R, D, 0, 0, None, st) == EINVAL
        torch.cuda.synchronize()
        assert ar.untouched(), "a rejected call wrote something"
    assert lib.raw("zs_mvn_max_dim") == 64
    assert [lib.raw("zs_mvn_group_lanes", n) for n in (0, 1, 2, 3, 5, 33, 64, 65)] == [0, 1, 2, 4, 8, 64, 64, 0]
