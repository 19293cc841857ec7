"""The planar and Householder flow stacks through the raw C ABI of libzs_nf.so (include/zs_nf.h), on the GPU.  See
tests/README_nf.md, which writes the tolerances out.

Truth: the header's arithmetic in numpy long double on the same float32-representable inputs (the float64 runs take them widened,
so one truth serves both); ``nf_host.reference_*`` -- the same formulas in torch float64, the truth of the module tests -- is held
against it.  An error bound is carried through the layers beside the truth (``planar_truth`` / ``householder_truth``): u = 2^-24
(2^-53 for _f64) per rounding, n u for an n-term sum, 2^-20 (2^-48) of the magnitude for a result through a library function.
Every case runs with aligned operands and with every operand shifted by one element: the two must agree bit for bit, and sentinel
elements around every output must survive.  The same call twice must give the same bits, P1f included."""
import numpy as np
import pytest
import torch

import nf_host
from kernel_abi import EINVAL, ENOTSUP, F32, F64, Arena, load, ptr, same_bits, sfx, stream

pytestmark = pytest.mark.gpu

LD = np.longdouble
DS = [1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 31, 32, 33, 40, 63, 64]
RS = [1, 3, 65]
LS = [1, 2, 5, 32]
WORST = {}          # quantity -> the worst error / tolerance seen in this session (printed; recorded in README_nf.md)


# ------------------------------------------------------------------------------------------------ inputs (CPU, float64)
def f32r(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def case_inputs(D, R, L):
    """float32-representable float64 operands, drawn in the order x, w, u, b, v, gy, gld: x ~ 2 N(0, 1); w, u ~ N(0, 1) / sqrt(D),
    u then moved along w so that w.u is -3 in layer 0 and +3 in the last layer (of a stack of more than one); b ~ N(0, 1);
    v ~ N(0, 1) with row 0 scaled by 1e-3 and the last row (of more than one) by 1e3; cotangents ~ N(0, 1)."""
    rng = np.random.default_rng(1000 * D + 10 * R + L)
    x = f32r(2.0 * rng.standard_normal((R, D)))
    w = f32r(rng.standard_normal((L, D)) / np.sqrt(D))
    u = rng.standard_normal((L, D)) / np.sqrt(D)
    for l, target in ([(0, -3.0)] + ([(L - 1, 3.0)] if L > 1 else [])):
        u[l] += (target - (w[l] * u[l]).sum()) * w[l] / (w[l] * w[l]).sum()
    b = f32r(rng.standard_normal(L))
    v = rng.standard_normal((L, R, D))
    v[:, 0] *= 1e-3
    if R > 1:
        v[:, R - 1] *= 1e3
    return dict(x=x, w=w, u=f32r(u), b=b, v=f32r(v), gy=f32r(rng.standard_normal((R, D))), gld=f32r(rng.standard_normal(R)))


def grid(D):
    return [(R, L) for R in RS for L in LS] + ([(4097, 2)] if D == 3 else [])


# ------------------------------------------------------------------------------------------------ truth and bounds (long double)
def units(dtype):
    return (LD(2.0) ** -24, LD(2.0) ** -20) if dtype == F32 else (LD(2.0) ** -53, LD(2.0) ** -48)


def planar_params_truth(u, w, U, LIB):
    D = u.shape[1]
    s, e_s = (w * u).sum(1), (D + 2) * U * np.abs(w * u).sum(1)
    n = (w * w).sum(1)
    e_n = (D + 2) * U * n
    sp = np.maximum(s, 0) + np.log1p(np.exp(-np.abs(s)))
    k = sp - 1 - s
    e_k = (LIB + 3 * U) * (sp + 1 + np.abs(s)) + 2 * e_s
    q = k[:, None] * w / n[:, None]
    e_q = np.abs(w) * (e_k / n)[:, None] + np.abs(q) * (e_n / n)[:, None] + (LIB + 3 * U) * np.abs(q)
    uh = u + q
    e_uh = e_q + 2 * U * (np.abs(u) + np.abs(q))
    c = (w * uh).sum(1)
    e_c = (D + 2) * U * np.abs(w * uh).sum(1) + (np.abs(w) * e_uh).sum(1)
    return dict(s=s, e_s=e_s, n=n, e_n=e_n, k=k, e_k=e_k, uh=uh, e_uh=e_uh, c=c, e_c=e_c)


def planar_truth(inp, dtype, n_wg, gy=True, gld=True):
    """value and bound of every output of P1, P1b and P1f: name -> (truth, tolerance)."""
    U, LIB = units(dtype)
    u, w, b, x = (inp[k].astype(LD) for k in ("u", "w", "b", "x"))
    (L, D), R = u.shape, x.shape[0]
    P = planar_params_truth(u, w, U, LIB)
    uh, e_uh, c, e_c = P["uh"], P["e_uh"], P["c"], P["e_c"]
    z, e_z = x, np.zeros_like(x)
    ld, e_ld = np.zeros(R, LD), np.zeros(R, LD)
    keep = []
    for l in range(L):
        wz = w[l] * z
        a = wz.sum(1) + b[l]
        e_a = (D + 2) * U * (np.abs(wz).sum(1) + abs(b[l])) + (np.abs(w[l]) * e_z).sum(1)
        t = np.tanh(a)
        e_t = LIB + e_a
        keep.append((z, e_z, t, e_t))
        ut = uh[l] * t[:, None]
        e_z = e_z + np.abs(uh[l]) * e_t[:, None] + e_uh[l] * np.abs(t)[:, None] + 2 * U * (np.abs(z) + np.abs(ut))
        z = z + ut
        h = 1 - t * t
        hc = h * c[l]
        m = np.abs(1 + hc)
        term = np.log(m)
        e_term = (abs(c[l]) * 2 * np.abs(t) * e_t + h * e_c[l] + 3 * U * (1 + np.abs(hc))) / m + LIB * np.abs(term)
        e_ld = e_ld + e_term + U * (np.abs(ld) + np.abs(term))
        ld = ld + term
    out = {"y": (z, e_z), "logdet": (ld, e_ld)}
    # the backward, downward
    g = inp["gy"].astype(LD) if gy else np.zeros((R, D), LD)
    gl = inp["gld"].astype(LD) if gld else np.zeros(R, LD)
    e_g = np.zeros((R, D), LD)
    S = {k: np.zeros(s, LD) for k, s in (("Guh", (L, D)), ("Gw", (L, D)), ("Gb", (L,)), ("Gc", (L,)))}
    E = {k: np.zeros_like(a) for k, a in S.items()}
    su = (R + n_wg + 2) * U
    for l in range(L - 1, -1, -1):
        zl, e_zl, t, e_t = keep[l]
        h = 1 - t * t
        e_h = 2 * np.abs(t) * e_t + e_t * e_t + 2 * U
        hc = h * c[l]
        m = 1 + hc
        e_m = abs(c[l]) * e_h + h * e_c[l] + 2 * U * (1 + np.abs(hc))
        r = c[l] / m
        e_r = e_c[l] / np.abs(m) + abs(c[l]) * e_m / (m * m) + (LIB + U) * np.abs(r)
        gu_ = g * uh[l]
        dot = gu_.sum(1)
        e_dot = (D + 2) * U * np.abs(gu_).sum(1) + (np.abs(g) * e_uh[l] + np.abs(uh[l]) * e_g).sum(1)
        t2 = gl * r * (-2 * t)
        e_t2 = np.abs(gl) * (e_r * 2 * np.abs(t) + np.abs(r) * 2 * e_t) + 3 * U * np.abs(t2)
        gt = dot + t2
        e_gt = e_dot + e_t2 + U * (np.abs(dot) + np.abs(t2))
        ga = gt * h
        e_ga = h * e_gt + np.abs(gt) * e_h + U * np.abs(ga)
        cu = g * t[:, None]
        e_cu = e_g * np.abs(t)[:, None] + np.abs(g) * e_t[:, None] + U * np.abs(cu)
        cw = ga[:, None] * zl
        e_cw = e_ga[:, None] * np.abs(zl) + np.abs(ga)[:, None] * e_zl + U * np.abs(cw)
        cc = gl * h / m
        e_cc = np.abs(gl) * (e_h / np.abs(m) + h * e_m / (m * m)) + (LIB + 2 * U) * np.abs(cc)
        for key, val, err in (("Guh", cu, e_cu), ("Gw", cw, e_cw), ("Gb", ga, e_ga), ("Gc", cc, e_cc)):
            S[key][l] = val.sum(0)
            E[key][l] = err.sum(0) + su * np.abs(val).sum(0)
        gaw = ga[:, None] * w[l]
        e_g = e_g + e_ga[:, None] * np.abs(w[l]) + 2 * U * (np.abs(g) + np.abs(gaw))
        g = g + gaw
    out["gx"] = (g, e_g)
    for key in S:
        out[key] = (S[key], E[key])
    # the parameter chain of P1f on those sums
    s, e_s, n, e_n, k, e_k = (P[key][:, None] for key in ("s", "e_s", "n", "e_n", "k", "e_k"))
    Gc, E_c = S["Gc"][:, None], E["Gc"][:, None]
    t1 = Gc * w
    Gu1 = S["Guh"] + t1
    e1 = E["Guh"] + E_c * np.abs(w) + 2 * U * (np.abs(S["Guh"]) + np.abs(t1))
    t2 = Gc * uh
    Gw1 = S["Gw"] + t2
    e2 = E["Gw"] + E_c * np.abs(uh) + np.abs(Gc) * e_uh + 2 * U * (np.abs(S["Gw"]) + np.abs(t2))
    p = (Gu1 * w).sum(1)[:, None]
    e_p = ((D + 2) * U * np.abs(Gu1 * w).sum(1) + (np.abs(w) * e1).sum(1))[:, None]
    dk = -1 / (1 + np.exp(s))
    e_dk = 2 * (LIB + U) * np.abs(dk) + LD(0.25) * e_s
    q = p / n
    e_q = e_p / n + np.abs(p) * e_n / (n * n) + (LIB + U) * np.abs(q)
    qs = q * dk
    e_qs = e_q * np.abs(dk) + np.abs(q) * e_dk + U * np.abs(qs)
    gu = Gu1 + qs * w
    e_gu = e1 + e_qs * np.abs(w) + 2 * U * (np.abs(Gu1) + np.abs(qs * w))
    kn = k / n
    e_kn = e_k / n + np.abs(k) * e_n / (n * n) + (LIB + U) * np.abs(kn)
    A = Gu1 * kn
    e_A = e1 * np.abs(kn) + np.abs(Gu1) * e_kn + U * np.abs(A)
    B = qs * u
    e_B = e_qs * np.abs(u) + U * np.abs(B)
    val = 2 * k * p / (n * n)
    e_val = 2 * (e_k * np.abs(p) + np.abs(k) * e_p) / (n * n) + np.abs(val) * (2 * e_n / n) + (LIB + 4 * U) * np.abs(val)
    C = val * w
    e_C = e_val * np.abs(w) + U * np.abs(C)
    gw = Gw1 + A + B - C
    e_gw = e2 + e_A + e_B + e_C + 3 * U * (np.abs(Gw1) + np.abs(A) + np.abs(B) + np.abs(C))
    out.update(gu=(gu, e_gu), gw=(gw, e_gw), gb=(S["Gb"], E["Gb"]))
    return out


def householder_truth(inp, dtype):
    U, LIB = units(dtype)
    v, x, g = inp["v"].astype(LD), inp["x"].astype(LD), inp["gy"].astype(LD)
    L, R, D = v.shape
    z, e_z = x, np.zeros_like(x)
    keep = []

    def ratio(num, e_num, n, e_n):          # num / n with the rule of a library division
        r = num / n
        return r, e_num / n + np.abs(num) * e_n / (n * n) + (LIB + U) * np.abs(r)

    def reflect(a, e_a, vl, dotv, e_dotv, n, e_n):
        r, e_r = ratio(dotv, e_dotv, n, e_n)
        upd = 2 * vl * r[:, None]
        return a - upd, e_a + 2 * np.abs(vl) * e_r[:, None] + U * np.abs(upd) + U * (np.abs(a) + np.abs(upd))

    def dot(vl, a, e_a):
        return (vl * a).sum(1), (D + 2) * U * np.abs(vl * a).sum(1) + (np.abs(vl) * e_a).sum(1)

    for l in range(L):
        n, e_n = dot(v[l], v[l], 0 * v[l])
        p, e_p = dot(v[l], z, e_z)
        keep.append((z, e_z, n, e_n, p, e_p))
        z, e_z = reflect(z, e_z, v[l], p, e_p, n, e_n)
    out = {"hy": (z, e_z)}
    e_g = np.zeros_like(g)
    gv, e_gv = np.zeros_like(v), np.zeros_like(v)
    for l in range(L - 1, -1, -1):
        zl, e_zl, n, e_n, p, e_p = keep[l]
        q, e_q = dot(v[l], g, e_g)
        pc, qc, nc = p[:, None], q[:, None], n[:, None]
        e_pc, e_qc, e_nc = e_p[:, None], e_q[:, None], e_n[:, None]
        A = pc * g + qc * zl
        e_A = e_pc * np.abs(g) + np.abs(pc) * e_g + e_qc * np.abs(zl) + np.abs(qc) * e_zl + 3 * U * (np.abs(pc * g) + np.abs(qc * zl))
        T1, e_T1 = ratio(-2 * A, 2 * e_A, nc, e_nc)
        Bv = 4 * pc * qc * v[l]
        e_B = 4 * np.abs(v[l]) * (e_pc * np.abs(qc) + np.abs(pc) * e_qc) + 3 * U * np.abs(Bv)
        n2 = nc * nc
        T2, e_T2 = ratio(Bv, e_B, n2, 2 * nc * e_nc + U * n2)
        gv[l] = T1 + T2
        e_gv[l] = e_T1 + e_T2 + U * (np.abs(T1) + np.abs(T2))
        g, e_g = reflect(g, e_g, v[l], q, e_q, n, e_n)
    out.update(hgx=(g, e_g), hgv=(gv, e_gv))
    return out


# ------------------------------------------------------------------------------------------------ device plumbing
@pytest.fixture(scope="module")
def lib():
    return load("nf")


def assert_close(name, got, truth, tol):
    got = got.cpu().to(F64).numpy().astype(LD).reshape(truth.shape)
    err = np.abs(got - truth)
    ratio = float((err / np.maximum(tol, LD(1e-300))).max()) if err.size else 0.0
    key = name.split(" [")[0]
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print("%s: worst error / tolerance = %.3f" % (name, ratio))
    assert bool(np.isfinite(got).all()), "%s: non-finite values" % name
    assert bool((err <= tol).all()), "%s: %d elements out of tolerance, worst error / tolerance %.3f" % (
        name, int((err > tol).sum()), ratio)


# ------------------------------------------------------------------------------------------------ raw calls
def call(lib, name, dtype, *args):
    return lib.raw(name + sfx(dtype), *args, stream())


def n_workgroups(lib, R, D):
    return lib.raw("zs_nf_planar_workgroups", R, D)


def run_planar(lib, dtype, inp, shift=0, gy=True, gld=True, want_y=True, want_ld=True, want_gx=True, want_partials=True,
               alias=False):
    """P1, P1b and P1f, each twice (bit-equal), guards checked: name -> device tensor (None where not asked for)."""
    ar = Arena(shift)
    u, w, b, x = (ar.put(inp[k], dtype) for k in ("u", "w", "b", "x"))
    (L, D), R = inp["u"].shape, inp["x"].shape[0]
    n_wg = n_workgroups(lib, R, D)
    gyt, gldt = ar.put(inp["gy"] if gy else None, dtype), ar.put(inp["gld"] if gld else None, dtype)
    res = {}
    for rep in range(2):
        if alias and rep == 1:          # the forward below overwrites x
            x = ar.put(inp["x"], dtype)
        gx = ar.out(R * D, dtype) if want_gx else None
        partials = ar.out(n_wg * L * (2 * D + 2), dtype) if want_partials else None
        assert call(lib, "zs_nf_planar_bwd", dtype, ptr(u), ptr(w), ptr(b), ptr(x), ptr(gyt), ptr(gldt), ptr(gx),
                    ptr(partials), R, D, L) == 0
        gu = gw = gb = None
        if want_partials:
            gu, gw, gb = ar.out(L * D, dtype), ar.out(L * D, dtype), ar.out(L, dtype)
            assert call(lib, "zs_nf_planar_finish", dtype, ptr(u), ptr(w), ptr(partials), n_wg, ptr(gu), ptr(gw), ptr(gb),
                        D, L) == 0
        y = x.view(-1) if alias else (ar.out(R * D, dtype) if want_y else None)
        ld = ar.out(R, dtype) if want_ld else None
        assert call(lib, "zs_nf_planar_fwd", dtype, ptr(u), ptr(w), ptr(b), ptr(x), ptr(y), ptr(ld), R, D, L) == 0
        torch.cuda.synchronize()
        now = dict(y=y, logdet=ld, gx=gx, partials=partials, gu=gu, gw=gw, gb=gb)
        for k, t in now.items():
            if rep == 1 and t is not None:
                assert same_bits(t, res[k]), "%s: the same call twice gave other bits" % k
        res = {k: (None if t is None else t.clone()) for k, t in now.items()}
    ar.check_guards()
    return res


def run_householder(lib, dtype, inp, shift=0, want_gx=True, want_gv=True, alias=False):
    ar = Arena(shift)
    v, x, gy = (ar.put(inp[k], dtype) for k in ("v", "x", "gy"))
    L, R, D = inp["v"].shape
    res = {}
    for rep in range(2):
        if alias and rep == 1:          # the forward below overwrites x
            x = ar.put(inp["x"], dtype)
        gx = ar.out(R * D, dtype) if want_gx else None
        gv = ar.out(L * R * D, dtype) if want_gv else None
        assert call(lib, "zs_nf_householder_bwd", dtype, ptr(v), ptr(x), ptr(gy), ptr(gx), ptr(gv), R, D, L) == 0
        y = x.view(-1) if alias else ar.out(R * D, dtype)
        assert call(lib, "zs_nf_householder_fwd", dtype, ptr(v), ptr(x), ptr(y), R, D, L) == 0
        torch.cuda.synchronize()
        now = dict(hy=y, hgx=gx, hgv=gv)
        for k, t in now.items():
            if rep == 1 and t is not None:
                assert same_bits(t, res[k]), "%s: the same call twice gave other bits" % k
        res = {k: (None if t is None else t.clone()) for k, t in now.items()}
    ar.check_guards()
    return res


def partial_sums(res, n_wg, L, D):
    """the four row sums of P1b from its partials, added in long double"""
    P = res["partials"].cpu().to(F64).numpy().astype(LD).reshape(n_wg, L, 2 * D + 2).sum(0)
    return dict(Guh=P[:, :D], Gw=P[:, D:2 * D], Gb=P[:, 2 * D], Gc=P[:, 2 * D + 1])


def check_case(lib, D, R, L, dtypes=(F32, F64), shifts=(0, 1)):
    inp = case_inputs(D, R, L)
    n_wg = n_workgroups(lib, R, D)
    tag = " [D=%d R=%d L=%d %%s]" % (D, R, L)
    for dtype in dtypes:
        truth = planar_truth(inp, dtype, n_wg)
        truth.update(householder_truth(inp, dtype))
        runs = []
        for shift in shifts:
            res = run_planar(lib, dtype, inp, shift)
            res.update(run_householder(lib, dtype, inp, shift))
            runs.append(res)
        for k in runs[0]:
            assert all(same_bits(runs[0][k], r[k]) for r in runs[1:]), "%s depends on the alignment of the operands" % k
        res = runs[0]
        for k in ("y", "logdet", "gx", "gu", "gw", "gb", "hy", "hgx", "hgv"):
            assert_close(k + tag % sfx(dtype), torch.as_tensor(res[k]), *truth[k])
        for k, got in partial_sums(res, n_wg, L, D).items():
            assert_close(k + tag % sfx(dtype), torch.from_numpy(got.astype(np.float64)), *truth[k])


# ------------------------------------------------------------------------------------------------ the tests
def test_abi_and_accessors(lib):
    assert lib.raw("zs_nf_max_dim") == 64 and lib.raw("zs_nf_max_layers") == 32 and lib.raw("zs_nf_max_workgroups") >= 1
    for D, G in ((1, 1), (2, 2), (3, 4), (5, 8), (9, 16), (17, 32), (33, 64), (64, 64), (0, 0), (65, 0)):
        assert lib.raw("zs_nf_group_lanes", D) == G
    cap = lib.raw("zs_nf_max_workgroups")
    assert n_workgroups(lib, 1, 40) == 1 and n_workgroups(lib, 65, 40) == 65 and n_workgroups(lib, 65, 3) == 5
    assert n_workgroups(lib, 10 ** 9, 1) == cap and n_workgroups(lib, 0, 3) == 0 and n_workgroups(lib, 5, 65) == 0


def test_the_truth_is_nf_hosts_reference():
    """the long-double truth of this file and the float64 ``nf_host.reference_*`` of the module tests are the same formulas"""
    inp = case_inputs(7, 5, 3)
    t = {k: torch.from_numpy(a) for k, a in inp.items()}
    truth = planar_truth(inp, F64, 1)
    truth.update(householder_truth(inp, F64))
    y, ld = nf_host.reference_planar_fwd(t["u"], t["w"], t["b"], t["x"])
    gx, Guh, Gw, Gb, Gc = nf_host.reference_planar_bwd(t["u"], t["w"], t["b"], t["x"], t["gy"], t["gld"])
    gu, gw, gb = nf_host.reference_planar_finish(t["u"], t["w"], Guh, Gw, Gb, Gc)
    hgx, hgv = nf_host.reference_householder_bwd(t["v"], t["x"], t["gy"])
    got = dict(y=y, logdet=ld, gx=gx, Guh=Guh, Gw=Gw, Gb=Gb, Gc=Gc, gu=gu, gw=gw, gb=gb, hgx=hgx, hgv=hgv,
               hy=nf_host.reference_householder_fwd(t["v"], t["x"]))
    for k, a in got.items():
        want = truth[k][0].astype(np.float64)
        assert np.allclose(a.numpy(), want, rtol=1e-9, atol=1e-9 * np.abs(want).max()), k


@pytest.mark.parametrize("D", DS)
def test_every_entry_point_against_the_truth(lib, D):
    for R, L in grid(D):
        check_case(lib, D, R, L)


def test_rows_past_the_capped_grid(lib):
    """P1, P1b + P1f, H1 and H1b with more rows than the capped grid covers in one pass: a workgroup walks a second tile, and P1b
    adds that tile to its own partials."""
    D, L = 1, 2
    R = lib.raw("zs_nf_max_workgroups") * (64 // lib.raw("zs_nf_group_lanes", D)) + 1
    assert n_workgroups(lib, R, D) == lib.raw("zs_nf_max_workgroups")
    check_case(lib, D, R, L, shifts=(0,))


def test_null_forms_and_aliasing_are_bit_equal(lib):
    inp = case_inputs(5, 65, 5)
    zero = dict(inp, gy=np.zeros_like(inp["gy"]), gld=np.zeros_like(inp["gld"]))
    for dtype in (F32, F64):
        full = run_planar(lib, dtype, inp)
        for kw, keys in ((dict(want_y=False), ("logdet",)), (dict(want_ld=False), ("y",)), (dict(want_gx=False), ("partials", "gu", "gw", "gb")),
                         (dict(want_partials=False), ("gx",)), (dict(alias=True), ("y", "logdet", "gx", "gu"))):
            part = run_planar(lib, dtype, inp, **kw)
            for k in keys:
                assert same_bits(part[k], full[k]), (kw, k)
        # a NULL cotangent means zero
        for kw, z in ((dict(gy=False), dict(inp, gy=zero["gy"])), (dict(gld=False), dict(inp, gld=zero["gld"]))):
            a, b = run_planar(lib, dtype, inp, **kw), run_planar(lib, dtype, z)
            for k in ("gx", "partials", "gu", "gw", "gb"):
                assert same_bits(a[k], b[k]), (kw, k)
        hfull = run_householder(lib, dtype, inp)
        assert same_bits(run_householder(lib, dtype, inp, want_gx=False)["hgv"], hfull["hgv"])
        assert same_bits(run_householder(lib, dtype, inp, want_gv=False)["hgx"], hfull["hgx"])
        assert same_bits(run_householder(lib, dtype, inp, alias=True)["hy"], hfull["hy"])


def test_a_zero_reflection_vector_gives_nan_in_its_row_only(lib):
    inp = case_inputs(5, 7, 3)
    bad = dict(inp, v=inp["v"].copy())
    bad["v"][1, 3] = 0.0
    for dtype in (F32, F64):
        a, b = run_householder(lib, dtype, inp), run_householder(lib, dtype, bad)
        rows = [r for r in range(7) if r != 3]
        for k in ("hy", "hgx"):
            x, y = a[k].reshape(7, 5), b[k].reshape(7, 5)
            assert bool(torch.isnan(y[3]).all()) and same_bits(x[rows], y[rows]), k
        x, y = a["hgv"].reshape(3, 7, 5), b["hgv"].reshape(3, 7, 5)
        assert bool(torch.isnan(y[:, 3]).all()) and same_bits(x[:, rows], y[:, rows])


def test_rejected_arguments_write_nothing_and_empty_shapes_launch_nothing(lib):
    inp = case_inputs(3, 3, 2)
    for dtype in (F32, F64):
        ar = Arena()
        u, w, b, x, v, gy, gld = (ar.put(inp[k], dtype) for k in ("u", "w", "b", "x", "v", "gy", "gld"))
        y, ld, gx, part, gu, gw, gb, gv = (ar.out(n, dtype) for n in (9, 3, 9, 16, 6, 6, 2, 18))
        p = ptr

        def fwd(u=u, w=w, b=b, x=x, y=y, ld=ld, R=3, D=3, L=2):
            return call(lib, "zs_nf_planar_fwd", dtype, p(u), p(w), p(b), p(x), p(y), p(ld), R, D, L)

        def bwd(u=u, w=w, b=b, x=x, gy=gy, gld=gld, gx=gx, part=part, R=3, D=3, L=2):
            return call(lib, "zs_nf_planar_bwd", dtype, p(u), p(w), p(b), p(x), p(gy), p(gld), p(gx), p(part), R, D, L)

        def fin(u=u, w=w, part=part, n_wg=1, gu=gu, gw=gw, gb=gb, D=3, L=2):
            return call(lib, "zs_nf_planar_finish", dtype, p(u), p(w), p(part), n_wg, p(gu), p(gw), p(gb), D, L)

        def hf(v=v, x=x, y=y, R=3, D=3, L=2):
            return call(lib, "zs_nf_householder_fwd", dtype, p(v), p(x), p(y), R, D, L)

        def hb(v=v, x=x, gy=gy, gx=gx, gv=gv, R=3, D=3, L=2):
            return call(lib, "zs_nf_householder_bwd", dtype, p(v), p(x), p(gy), p(gx), p(gv), R, D, L)

        for f in (fwd, bwd, hf, hb):
            assert f(D=0) == EINVAL and f(R=-1) == EINVAL and f(L=-1) == EINVAL and f(x=None) == EINVAL
            assert f(D=65) == ENOTSUP and f(L=33) == ENOTSUP
            assert f(R=0) == 0 and f(L=0) == 0
        for f in (fwd, bwd):
            assert f(u=None) == EINVAL and f(w=None) == EINVAL and f(b=None) == EINVAL
        assert fwd(y=None, ld=None) == EINVAL
        assert bwd(gy=None, gld=None) == EINVAL and bwd(gx=None, part=None) == EINVAL
        assert fin(u=None) == EINVAL and fin(w=None) == EINVAL and fin(part=None) == EINVAL and fin(D=0) == EINVAL
        assert fin(L=-1) == EINVAL and fin(gu=None, gw=None, gb=None) == EINVAL and fin(D=65) == ENOTSUP and fin(L=33) == ENOTSUP
        assert fin(n_wg=0) == EINVAL and fin(n_wg=lib.raw("zs_nf_max_workgroups") + 1) == EINVAL and fin(L=0) == 0
        assert hf(v=None) == EINVAL and hf(y=None) == EINVAL
        assert hb(v=None) == EINVAL and hb(gy=None) == EINVAL and hb(gx=None, gv=None) == EINVAL
        torch.cuda.synchronize()
        assert ar.untouched()


def test_print_the_worst_ratios():
    for k in sorted(WORST):
        print("worst error / tolerance  %-8s %.3f" % (k, WORST[k]))
