"""The inclusive-KL kernels through the raw C ABI of libzs_klpq.so (include/zs_klpq.h), on the GPU.  See tests/README_klpq.md.

Truth: tests/klpq_host.py ``reference_*`` -- the header's formulas in float64 -- on the same inputs (the float64 runs take the
float32-representable inputs widened, so one truth serves both).  Every case runs with aligned operands and with every operand
shifted by one element, in its own layout and with every term in the opposite layout (shared terms spelled out): all four must
agree bit for bit, sentinel elements around every output must survive, and the same calls again must give the same bits.  The
launch with the batch mean (one workgroup) and the launch without it (many) must agree on ``bound`` and ``ess`` bit for bit.

Tolerances (derived, not tuned; u = 2^-24 for _f32, 2^-53 for _f64; tiny = the smallest normal number of the format):
  e_kb  = (Tp + Tq) u sum_t |term_t[k, b]|                    the two left-to-right sums and their difference;  E_b = max_k e_kb
  r_b   = 2 E_b + (8 + K) u                                   relative error of a weight: its own exponent and the largest one
                                                              (each also covers the rounding of lw_k - m), exp, the K-term sum, the divide
  w      r_b w + tiny
  bound  E_b + (8 + K) u + 4 u (|m| + |log s| + log K)
  cost   sum_k w_k (r_b |x_k| + e_kb) + (K + 4) u sum_k |w_k x_k| + tiny        x = lq (+ lp with the model_grad flag)
  ess    ess (2 r_b + (K + 4) u)
  mean   (sum_b tol(cost_b) + (B / 64 + 10) u sum_b |cost_b|) / B
  g      (r_b + 4 u) (|gc| + |gb|) w + tiny ;  a broadcast sum over n elements: the sum of those + (n + 2) u sum |terms|
A particle with lp = -inf must have weight exactly 0.  The float32 torch composition of the same formulas on the CPU is held to
the same bounds for every case (not gpu): a bound it violated would be too tight to blame on the kernel."""
import math

import numpy as np
import pytest
import torch

import klpq_host
from kernel_abi import EINVAL, ENOTSUP, F32, F64, Arena, load, ptr, same_bits, sfx, stream, unit, untouched

gpu = pytest.mark.gpu

MODEL_GRAD, BOUND_ONLY, GCOST_MEAN = 1, 2, 4
KS = [1, 2, 3, 5, 31, 32, 33, 50, 63, 64, 65, 130, 257]
BS = [1, 3, 65, 257]
MAX_TERMS = 8
MEAN_MAX_B = 1024
TERMS = [(1, 1), (2, 1), (3, 2), (MAX_TERMS, MAX_TERMS)]
LAYOUTS = ["kb", "bk", "mixed", "sb0", "sk0"]
SCALES = [0.0, 1.0, 5.0]
WORST = {}          # quantity -> the worst error / tolerance seen in this session (printed; recorded in README_klpq.md)


# ------------------------------------------------------------------------------------------------ inputs (CPU, float64)
def f32r(a):
    return torch.from_numpy(np.asarray(a).astype(np.float32).astype(np.float64))


def cases_of(K):
    """(B, Tp, Tq, layout, scale) for this K: every B x (Tp, Tq) x layout, the scale cycling so that each layout and each
    (Tp, Tq) meets each scale."""
    out = []
    for bi, B in enumerate(BS + ([4097] if K == 3 else [])):
        for ti, (Tp, Tq) in enumerate(TERMS):
            for li, layout in enumerate(LAYOUTS):
                out.append((B, Tp, Tq, layout, SCALES[(bi + ti + li) % 3]))
    return out


def case_inputs(K, B, Tp, Tq, layout, scale):
    """float32-representable float64 terms, each of logical shape [K, B], [K, 1] (shared by the batch) or [1, B] (shared by the
    particles): scale N(0, 1) - 1; datapoint 0 is offset by +80 and datapoint 1 by -80 in the first generator term, and one
    particle of the last datapoint has lp = -inf (K > 1); a shared term is a row or the last column of such a matrix.
    Cotangents ~ N(0, 1)."""
    rng = np.random.default_rng(100000 * K + 100 * B + 10 * Tp + LAYOUTS.index(layout))
    p = [scale * rng.standard_normal((K, B)) - 1.0 for _ in range(Tp)]
    q = [scale * rng.standard_normal((K, B)) - 1.0 for _ in range(Tq)]
    p[0][:, 0] += 80.0
    if B > 1:
        p[0][:, 1] -= 80.0
    if K > 1:
        p[0][K // 2, B - 1] = -np.inf
    if layout == "sb0":          # (the last column: with a single generator term it is the one that holds the -inf)
        p[-1] = p[-1][:, B - 1:]
    if layout == "sk0":
        q[-1] = q[-1][:1, :]
    return dict(p=[f32r(t) for t in p], q=[f32r(t) for t in q], gcost=f32r(rng.standard_normal(B)), gbound=f32r(rng.standard_normal(B)),
                gmean=f32r(rng.standard_normal(1)))


def storage(layout, side, i, n, flipped):
    """'kb' or 'bk': how term i of n of a side is stored."""
    if layout in ("kb", "sb0"):
        s = "kb"
    elif layout in ("bk", "sk0"):
        s = "bk"
    else:
        s = "kb" if (i + (side == "q")) % 2 == 0 else "bk"
    return ("bk" if s == "kb" else "kb") if flipped else s


# ------------------------------------------------------------------------------------------------ the bounds
def tiny(dtype):
    return 2.0 ** -126 if dtype == F32 else 2.0 ** -1022


class Bounds(object):
    """The bounds of the module docstring for one case and dtype, in float64 on the CPU."""

    def __init__(self, dtype, d, K, B, model_grad):
        u, self.tiny = unit(dtype), tiny(dtype)
        self.u, self.K, self.B = u, K, B
        r = klpq_host.reference_forward(d["p"], d["q"], K, B, model_grad)
        self.r = r
        mag = sum(t.abs().expand(K, B) for t in d["p"] + d["q"])
        e = (len(d["p"]) + len(d["q"])) * u * mag                                   # [K, B]
        live = torch.isfinite(r["lw"])
        self.live = live
        self.e = torch.where(live, e, torch.zeros_like(e))
        self.E = self.e.max(0).values                                               # [B]
        self.rel = 2 * self.E + (8 + K) * u                                         # [B]
        wt = r["w"].t()                                                             # [K, B]
        x = r["lq"] + r["lp"] if model_grad else r["lq"]
        wx = torch.where(wt == 0, torch.zeros_like(wt), (wt * x).abs())
        ax = torch.where(wt == 0, torch.zeros_like(wt), x.abs())
        self.w = (self.rel[None] * wt + self.tiny).t()                              # [B, K]
        m = r["lw"].max(0).values
        logs = r["bound"] + math.log(K) - m
        self.bound = self.E + (8 + K) * u + 4 * u * (m.abs() + logs.abs() + math.log(K))
        self.cost = (wt * (self.rel[None] * ax + self.e)).sum(0) + (K + 4) * u * wx.sum(0) + self.tiny
        self.ess = r["ess"] * (2 * self.rel + (K + 4) * u)
        self.mean = (self.cost.sum() + (B / 64.0 + 10) * u * r["cost"].abs().sum()) / B

    def grads(self, gc, gb):
        """(tolerance [K, B] of a full term's gradient, |terms| [K, B]) for cotangents gc, gb [B]"""
        wt = self.r["w"].t()
        mag = (gc.abs() + gb.abs())[None] * wt
        return (self.rel[None] + 4 * self.u) * mag + self.tiny, mag

    def reduced(self, tol, mag, shape):
        """the tolerance of the gradient of a term of ``shape``: summed over the shared axes, plus the sum's own rounding"""
        n = 1
        for dmn in (0, 1):
            if shape[dmn] == 1 and tol.shape[dmn] != 1:
                n *= tol.shape[dmn]
                tol, mag = tol.sum(dmn, keepdim=True), mag.sum(dmn, keepdim=True)
        return tol + ((n + 2) * self.u * mag if n > 1 else 0.0)


def in_dtype_sum(terms, dtype, K, B):
    total = None
    for t in terms:
        t = t.to(dtype).expand(K, B)
        total = t if total is None else total + t
    return total


def ratio_of(name, got, truth, tol):
    got, truth = got.detach().cpu().to(F64).reshape(truth.shape), truth.to(F64)
    tol = torch.as_tensor(tol, dtype=F64).expand_as(truth)
    err = (got - truth).abs()
    err = torch.where(got == truth, torch.zeros_like(err), err)          # (equal infinities)
    ratio = float((err / tol.clamp(min=1e-320)).max()) if err.numel() else 0.0
    key = name.split(" [")[0]
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    return ratio, err, tol


def assert_close(name, got, truth, tol):
    ratio, err, tol = ratio_of(name, got, truth, tol)
    print("%s: worst error / tolerance = %.3f" % (name, ratio))
    assert not bool(torch.isnan(got).any()), "%s: NaN" % name
    assert bool((err <= tol).all()), "%s: %d elements out of tolerance, worst error / tolerance %.3f" % (name, int((err > tol).sum()), ratio)


def check_case(tag, dtype, d, K, B, res, mean_expected):
    """``res``: dict of the outputs of one case, CPU tensors in logical shapes (gradients [K or 1, B or 1])."""
    b0, b1 = Bounds(dtype, d, K, B, False), Bounds(dtype, d, K, B, True)
    r0, r1 = b0.r, b1.r
    assert_close("w" + tag, res["w"], r0["w"], b0.w)
    dead = ~b0.live.t()
    assert bool((res["w"].reshape(B, K)[dead] == 0).all()), "a particle with lp = -inf must have weight exactly 0" + tag
    assert_close("cost" + tag, res["cost"], r0["cost"], b0.cost)
    assert_close("bound" + tag, res["bound"], r0["bound"], b0.bound)
    assert_close("ess" + tag, res["ess"], r0["ess"], b0.ess)
    assert_close("cost (model_grad)" + tag, res["cost_mg"], r1["cost"], b1.cost)
    if mean_expected:
        assert_close("mean_cost" + tag, res["mean"], r0["mean"], b0.mean)
    if K == 1:
        lw = in_dtype_sum(d["p"], dtype, K, B) - in_dtype_sum(d["q"], dtype, K, B)          # the kernel's own lw: IEEE sums, left to right
        assert bool((res["w"].reshape(-1) == 1).all()) and bool((res["ess"].reshape(-1) == 1).all()), "K = 1: w = 1, ess = 1" + tag
        assert torch.equal(res["bound"].reshape(-1).to(dtype), lw.reshape(-1)), "K = 1: bound = lw" + tag
    # backward A: gcost [B] and gbound [B], no model_grad;  backward B: the mean's cotangent, model_grad
    gq, gp = klpq_host.reference_backward(r0["w"], d["gcost"], d["gbound"], False, B)
    tol, mag = b0.grads(d["gcost"], d["gbound"])
    for side, terms, g in (("q", d["q"], gq), ("p", d["p"], gp)):
        for i, t in enumerate(terms):
            shape = tuple(t.shape)
            assert_close("grad" + tag, res["gA_%s%d" % (side, i)], klpq_host.reduce_to(g, shape), b0.reduced(tol, mag, shape))
    gq, gp = klpq_host.reference_backward(r0["w"], d["gmean"], None, True, B, gcost_is_mean=True)
    gc = (d["gmean"] / B).expand(B)
    tol, mag = b0.grads(gc, torch.zeros(B, dtype=F64))
    for side, terms, g in (("q", d["q"], gq), ("p", d["p"], gp)):
        for i, t in enumerate(terms):
            if side == "q" and i == 0:
                continue          # (handed a NULL gradient pointer: skipped)
            shape = tuple(t.shape)
            assert_close("grad (mean)" + tag, res["gB_%s%d" % (side, i)], klpq_host.reduce_to(g, shape), b0.reduced(tol, mag, shape))


# ------------------------------------------------------------------------------------------------ the CPU cross-check (not gpu)
def torch_f32_results(d, K, B):
    """The same formulas with float32 torch operations on the CPU, the terms added left to right."""
    def run(model_grad):
        p = [t.to(F32).expand(K, B) for t in d["p"]]
        q = [t.to(F32).expand(K, B) for t in d["q"]]
        lp, lq = p[0], q[0]
        for t in p[1:]:
            lp = lp + t
        for t in q[1:]:
            lq = lq + t
        lw = lp - lq
        m = lw.max(0, keepdim=True).values
        e = torch.exp(lw - m)
        s = e.sum(0, keepdim=True)
        w = e / s
        x = lq + lp if model_grad else lq
        cost = -torch.where(w == 0, torch.zeros_like(w), w * x).sum(0)
        return w, cost, (m + torch.log(s))[0] - F32_LOG(K), 1.0 / (w * w).sum(0)
    w, cost, bound, ess = run(False)
    res = dict(w=w.t().contiguous(), cost=cost, bound=bound, ess=ess, cost_mg=run(True)[1], mean=cost.mean())
    gc, gb, gm = d["gcost"].to(F32), d["gbound"].to(F32), d["gmean"].to(F32)
    for name, c, b_, mg in (("gA", gc, gb, False), ("gB", (gm / B).expand(B), torch.zeros(B), True)):
        gq = -c[None] * w - b_[None] * w
        gp = (-c[None] * w + b_[None] * w) if mg else b_[None] * w
        for side, terms, g in (("q", d["q"], gq), ("p", d["p"], gp)):
            for i, t in enumerate(terms):
                res["%s_%s%d" % (name, side, i)] = klpq_host.reduce_to(g, tuple(t.shape))
    return res


def F32_LOG(K):
    return float(np.float32(math.log(K)))


@pytest.mark.parametrize("K", KS)
def test_float32_torch_composition_stays_inside_the_bounds(K):
    for B, Tp, Tq, layout, scale in cases_of(K):
        d = case_inputs(K, B, Tp, Tq, layout, scale)
        tag = " [torch f32: K=%d B=%d Tp=%d Tq=%d %s scale %g]" % (K, B, Tp, Tq, layout, scale)
        check_case(tag, F32, d, K, B, torch_f32_results(d, K, B), True)
    print("worst error / tolerance so far: %s" % ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


# ------------------------------------------------------------------------------------------------ device plumbing
@pytest.fixture(scope="module")
def lib():
    return load("klpq")


def term_row(row, t, val, store, ar, dtype, want_grad):
    """Fill table row ``row`` for logical term t ([K, B], [K, 1] or [1, B]) whose values sit in ``val`` as 'kb' or 'bk'; returns
    (grad buffer or None, a function that turns the flat grad buffer into the logical shape)."""
    k, b = t.shape
    sk, sb = (b, 1) if store == "kb" else (1, k)
    row.value = val.data_ptr()
    row.sk, row.sb = (0 if k == 1 else sk), (0 if b == 1 else sb)
    grad = ar.out(k * b, dtype) if want_grad else None
    row.grad = ptr(grad)

    def logical(g):
        g = g.cpu()
        return g.view(k, b) if store == "kb" else g.view(b, k).t()
    return grad, logical


def run_case(lib, dtype, d, K, B, layout, shift, flipped):
    """Every launch of a case (in its own layout and alignment twice: bit-equal); returns the dict of CPU results in logical shapes."""
    from zhusuan._klpq_hip import KlpqTerm
    ar = Arena(shift)
    Tp, Tq = len(d["p"]), len(d["q"])
    terms = {"p": d["p"], "q": d["q"]}
    if flipped:          # every term in the opposite layout, shared terms spelled out
        terms = {s: [t.expand(K, B) for t in ts] for s, ts in terms.items()}
    st = stream()
    gcost, gbound, gmean = ar.put(d["gcost"], dtype), ar.put(d["gbound"], dtype), ar.put(d["gmean"], dtype)
    with_mean = B <= MEAN_MAX_B

    vals = {}
    for side, n in (("p", Tp), ("q", Tq)):          # the values go to the device once; every table gets gradient buffers of its own
        for i, t in enumerate(terms[side]):
            store = storage(layout, side, i, n, flipped)
            vals[side, i] = (ar.put((t if store == "kb" else t.t()).contiguous(), dtype), store)

    def tables(null_first_q):
        tabs, grads = {}, {}
        for side, n in (("p", Tp), ("q", Tq)):
            tab = (KlpqTerm * n)()
            for i, t in enumerate(terms[side]):
                want = not (null_first_q and side == "q" and i == 0)
                val, store = vals[side, i]
                g, logical = term_row(tab[i], t, val, store, ar, dtype, want)
                if want:
                    grads["%s%d" % (side, i)] = (g, logical)
            tabs[side] = tab
        return tabs, grads

    res = {}
    for rep in range(2 if (shift == 0 and not flipped) else 1):          # the same calls again, once per case: the same bits
        tabs, _ = tables(False)
        w, cost, bound, ess = ar.out(B * K, dtype), ar.out(B, dtype), ar.out(B, dtype), ar.out(B, dtype)
        mean = ar.out(1, dtype) if with_mean else None
        rc = lib.raw("zs_klpq_forward" + sfx(dtype), tabs["p"], Tp, tabs["q"], Tq, K, B, 0, ptr(w), ptr(cost), ptr(bound), ptr(ess),
                     ptr(mean), st)
        assert rc == 0
        cost_mg, bound2, ess2 = ar.out(B, dtype), ar.out(B, dtype), ar.out(B, dtype)
        rc = lib.raw("zs_klpq_forward" + sfx(dtype), tabs["p"], Tp, tabs["q"], Tq, K, B, MODEL_GRAD, None, ptr(cost_mg), ptr(bound2),
                     ptr(ess2), None, st)
        assert rc == 0
        tabA, gA = tables(False)
        rc = lib.raw("zs_klpq_backward" + sfx(dtype), tabA["p"], Tp, tabA["q"], Tq, K, B, 0, ptr(w), ptr(gcost), ptr(gbound), st)
        assert rc == 0
        tabB, gB = tables(True)          # (the first variational term hands in a NULL gradient pointer)
        rc = lib.raw("zs_klpq_backward" + sfx(dtype), tabB["p"], Tp, tabB["q"], Tq, K, B, MODEL_GRAD | GCOST_MEAN, ptr(w), ptr(gmean),
                     None, st)
        assert rc == 0
        torch.cuda.synchronize()
        out = dict(w=w.cpu().view(B, K), cost=cost.cpu(), bound=bound.cpu(), ess=ess.cpu(), cost_mg=cost_mg.cpu())
        if with_mean:
            out["mean"] = mean.cpu().view(())
        for k_, (g, logical) in gA.items():
            out["gA_" + k_] = logical(g)
        for k_, (g, logical) in gB.items():
            out["gB_" + k_] = logical(g)
        assert same_bits(bound, bound2) and same_bits(ess, ess2), "one workgroup and many disagree on bound / ess"
        if rep == 0:
            res = out
        else:
            for name in res:
                assert same_bits(res[name], out[name]), "two identical calls differ in %s" % name
    ar.check_guards()
    return res


@gpu
@pytest.mark.parametrize("K", KS)
def test_forward_and_backward_against_float64(lib, K):
    for B, Tp, Tq, layout, scale in cases_of(K):
        d = case_inputs(K, B, Tp, Tq, layout, scale)
        for dtype in (F32, F64):
            runs = [run_case(lib, dtype, d, K, B, layout, shift, flipped) for shift in (0, 1) for flipped in (False, True)]
            ref = runs[0]
            for other in runs[1:]:
                for name in ref:
                    if tuple(other[name].shape) == tuple(ref[name].shape):          # (a shared term's gradient is [K, B] when spelled out)
                        assert same_bits(ref[name], other[name]), "%s differs between layouts / alignments (K=%d B=%d %s)" % (name, K, B, layout)
            tag = " [K=%d B=%d Tp=%d Tq=%d %s scale %g %s]" % (K, B, Tp, Tq, layout, scale, sfx(dtype))
            check_case(tag, dtype, d, K, B, ref, B <= MEAN_MAX_B)
    print("worst error / tolerance so far: %s" % ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))


def simple_tables(ar, dtype, d, K, B, grads=False):
    from zhusuan._klpq_hip import KlpqTerm
    tabs, keep = {}, []
    for side in ("p", "q"):
        tab = (KlpqTerm * len(d[side]))()
        for i, t in enumerate(d[side]):
            val = ar.put(t.contiguous(), dtype)
            keep.append((val, term_row(tab[i], t, val, "kb", ar, dtype, grads)))
        tabs[side] = tab
    return tabs, keep


@gpu
def test_a_row_of_all_minus_infinity_gives_nan_there_and_leaves_its_neighbours_alone(lib):
    K, B = 5, 65
    d = case_inputs(K, B, 2, 1, "kb", 1.0)
    bad = dict(d, p=[d["p"][0].clone(), d["p"][1]])
    bad["p"][0][:, 7] = -math.inf
    for dtype in (F32, F64):
        outs = []
        for case in (d, bad):
            ar = Arena(0)
            tabs, keep = simple_tables(ar, dtype, case, K, B)
            o = [ar.out(B * K, dtype), ar.out(B, dtype), ar.out(B, dtype), ar.out(B, dtype), ar.out(1, dtype)]
            assert lib.raw("zs_klpq_forward" + sfx(dtype), tabs["p"], 2, tabs["q"], 1, K, B, 0, *[ptr(t) for t in o], stream()) == 0
            ar.check_guards()
            outs.append([o[0].cpu().view(B, K)] + [t.cpu() for t in o[1:]])
        good, hit = outs
        others = [b for b in range(B) if b != 7]
        for a, b in zip(good[:4], hit[:4]):
            assert bool(torch.isnan(b[7]).all()), "the all -inf row is not NaN"
            assert same_bits(a[others], b[others]), "a neighbour of the all -inf row changed"
        assert bool(torch.isnan(hit[4]).all()) and bool(torch.isfinite(good[4]).all())


@gpu
def test_bound_only_and_null_outputs(lib):
    K, B = 33, 65
    d = case_inputs(K, B, 3, 2, "kb", 1.0)
    for dtype in (F32, F64):
        ar = Arena(0)
        tabs, keep = simple_tables(ar, dtype, d, K, B)
        name, st = "zs_klpq_forward" + sfx(dtype), stream()
        full = [ar.out(B * K, dtype), ar.out(B, dtype), ar.out(B, dtype), ar.out(B, dtype), ar.out(1, dtype)]
        assert lib.raw(name, tabs["p"], 3, tabs["q"], 2, K, B, 0, *[ptr(t) for t in full], st) == 0
        # bound_only writes only bound, whatever else is handed in
        only = [ar.out(B * K, dtype), ar.out(B, dtype), ar.out(B, dtype), ar.out(B, dtype), ar.out(1, dtype)]
        assert lib.raw(name, tabs["p"], 3, tabs["q"], 2, K, B, BOUND_ONLY, *[ptr(t) for t in only], st) == 0
        alone = ar.out(B, dtype)
        assert lib.raw(name, tabs["p"], 3, tabs["q"], 2, K, B, BOUND_ONLY, None, None, ptr(alone), None, None, st) == 0
        assert lib.raw(name, tabs["p"], 3, tabs["q"], 2, K, B, BOUND_ONLY, ptr(only[0]), None, None, None, None, st) == EINVAL
        # each output alone: the others NULL
        singles = []
        for i in range(5):
            o = ar.out(full[i].numel(), dtype)
            args = [None] * 5
            args[i] = ptr(o)
            assert lib.raw(name, tabs["p"], 3, tabs["q"], 2, K, B, 0, *args, st) == 0
            singles.append(o)
        ar.check_guards()
        assert same_bits(only[2], full[2]) and same_bits(alone, full[2])
        for i in (0, 1, 3, 4):
            assert untouched(only[i]), "bound_only wrote something besides bound"
        for a, b in zip(singles, full):
            assert same_bits(a, b), "an output alone differs from the same output among the others"


@gpu
def test_rejected_arguments_write_nothing(lib):
    from zhusuan._klpq_hip import KlpqTerm
    K, B = 5, 3
    d = case_inputs(K, B, 2, 2, "kb", 1.0)
    for dtype in (F32, F64):
        ar = Arena(0)
        tabs, keep = simple_tables(ar, dtype, d, K, B, grads=True)
        big = (KlpqTerm * (MAX_TERMS + 1))()
        for i in range(MAX_TERMS + 1):
            big[i] = tabs["p"][0]
        hole = (KlpqTerm * 2)()
        hole[0], hole[1] = tabs["p"][0], tabs["p"][1]
        hole[1].value = None
        nograd = (KlpqTerm * 2)()
        for i in range(2):
            nograd[i] = tabs["q"][i]
            nograd[i].grad = None
        o = [ar.out(B * K, dtype), ar.out(B, dtype), ar.out(B, dtype), ar.out(B, dtype), ar.out(1, dtype)]
        w, gc = ar.put(torch.full((B, K), 0.2, dtype=F64), dtype), ar.put(d["gcost"], dtype)
        po, st, s = [ptr(t) for t in o], stream(), sfx(dtype)

        def fwd(p, tp, q, tq, k, b, flags=0, outs=po):
            return lib.raw("zs_klpq_forward" + s, p, tp, q, tq, k, b, flags, *outs, st)

        def bwd(p, tp, q, tq, k, b, w_=w, gc_=gc):
            return lib.raw("zs_klpq_backward" + s, p, tp, q, tq, k, b, 0, ptr(w_), ptr(gc_), None, st)
        P, Q = tabs["p"], tabs["q"]
        for f in (fwd, bwd):
            assert f(P, 0, Q, 2, K, B) == EINVAL and f(P, 2, Q, 0, K, B) == EINVAL and f(P, -1, Q, 2, K, B) == EINVAL
            assert f(big, MAX_TERMS + 1, Q, 2, K, B) == ENOTSUP and f(P, 2, big, MAX_TERMS + 1, K, B) == ENOTSUP
            assert f(None, 2, Q, 2, K, B) == EINVAL and f(P, 2, None, 2, K, B) == EINVAL
            assert f(P, 2, Q, 2, -1, B) == EINVAL and f(P, 2, Q, 2, K, -1) == EINVAL
            assert f(P, 2, Q, 2, 0, B) == 0 and f(P, 2, Q, 2, K, 0) == 0          # K B == 0 launches nothing
        assert fwd(P, 2, Q, 2, K, B, outs=[None] * 5) == EINVAL                    # nothing to write
        assert fwd(hole, 2, Q, 2, K, B) == EINVAL                                  # a term without a value
        assert fwd(P, 2, Q, 2, K, MEAN_MAX_B + 1) == ENOTSUP                       # the batch mean beyond one workgroup
        assert bwd(P, 2, Q, 2, K, B, w_=None) == EINVAL and bwd(P, 2, Q, 2, K, B, gc_=None) == EINVAL
        assert bwd(nograd, 2, nograd, 2, K, B) == EINVAL                           # no gradient asked for
        torch.cuda.synchronize()
        assert ar.untouched(), "a rejected call wrote something"
    assert lib.raw("zs_klpq_max_terms") == MAX_TERMS and lib.raw("zs_klpq_mean_max_batch") == MEAN_MAX_B
    assert [lib.raw("zs_klpq_group_lanes", n) for n in (0, 1, 2, 3, 5, 33, 64, 65, 257)] == [0, 1, 2, 4, 8, 64, 64, 64, 64]
