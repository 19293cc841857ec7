"""The SVGD kernels through the raw C ABI of libzs_svgd.so (include/zs_svgd.h), on the GPU.  See tests/README_svgd.md.

Truth: the header's formulas in float64 torch on the CPU (``truth`` below, distances from differences), on float32-representable
inputs, so one truth serves _f32 and _f64.  Reference: ``zhusuan.mcmc.SVGD.torch_step``, the torch composition of the same
formulas, run on the CPU in the kernel's element type.  With e = max |reference - truth| over a case's array, a kernel result may
deviate from the truth, in every element, by at most max(RATIO e, 16 unit max|truth|) -- phi and the kernel matrix each with
their own e.  phi is read off the moved particles: q_out = theta + STEP phi with STEP = 64, so the rounding of the stored sum, at
most 2 unit |q_out|, is STEP times smaller against phi than the particles' own magnitude; that term is added to STEP times phi's
bound and nothing else is."""
import math

import numpy as np
import pytest
import torch

from kernel_abi import DEV, EINVAL, ENOTSUP, F32, F64, Arena, covered, load, ptr, same_bits, sfx, stream, unit

from zhusuan import _svgd_hip as B
from zhusuan.mcmc.SVGD import precondition, torch_step

RATIO = 4
STEP = 64.0
SLAB, CAP = B.SLAB, B.GRID_CAP
LAYOUTS = {"one": [1], "three": [3], "edge": [SLAB - 1, SLAB + 1], "cross": [5, SLAB, 2],
           "walk": [SLAB * CAP + 7, 2 * SLAB - 3]}          # 131 slabs on 128 workgroups: the cap is reached, three walk two slabs
# (K, layout, mu); K = 0 stands for the element type's cap.  Every K, every layout and both mu appear.
CASES = [(1, "three", 0), (2, "one", 0), (15, "edge", 100), (16, "cross", 0), (17, "walk", 100), (33, "cross", 100), (65, "edge", 0),
         (0, "three", 0), (0, "edge", 100)]


def inputs(K, layout, mu, seed=0):
    rng = np.random.default_rng(1000 * K + 10 * len(layout) + mu + seed)
    f32r = lambda a: torch.from_numpy(a.astype(np.float32).astype(np.float64))
    return [f32r(mu + rng.standard_normal((K, m))) for m in layout], [f32r(rng.standard_normal((K, m))) for m in layout]


def truth(thetas, grads, bandwidth=None):
    """(phi list, kernel, h) in float64"""
    th, g = torch.cat(thetas, 1), torch.cat(grads, 1)
    K = th.shape[0]
    d = torch.stack([((th[i] - th) ** 2).sum(1) for i in range(K)])
    med = float(np.median(d.numpy()))
    h = bandwidth if bandwidth is not None else (med / math.log(K + 1) if med > 0 else 1.0)
    k = torch.exp(-d / h)
    phi = (k.t() @ g + (2 / h) * (k.sum(0)[:, None] * th - k.t() @ th)) / K
    return list(phi.split([t.shape[1] for t in thetas], 1)), k, h


def bounds(dtype, thetas, grads, t, bandwidth=None):
    """the tolerances of phi, of the kernel matrix and of h for this case, from the reference's own error"""
    phis, k, h = torch_step([a.to(dtype) for a in thetas], [a.to(dtype) for a in grads], bandwidth)
    ephi = max(float((a.double() - b).abs().max()) for a, b in zip(phis, t[0]))
    top = max(float(b.abs().max()) for b in t[0])
    return (max(RATIO * ephi, 16 * unit(dtype) * top), max(RATIO * float((k - t[1]).abs().max()), 16 * unit(dtype)),
            max(RATIO * abs(float(h) - t[2]), 16 * unit(dtype) * t[2]))


def cap_of(dtype):
    return B.MAX_PARTICLES[4 if dtype == F32 else 8]


def table(K, q, g=None, out=None, h=None):
    cols = dict(q_in=q, grad=g, q_out=out, h=h)
    tb = (B.SvgdTensor * len(q))()
    start = 0
    for i, e in enumerate(tb):
        for name, col in cols.items():
            if col is not None:
                setattr(e, name, ptr(col[i]))
        e.start, e.row = start, q[i].shape[1]
        start += q[i].numel()
    return tb, start


def step(lib, dtype, ar, K, q, g, bandwidth=None, alias=False, h=None, first=True, step_size=STEP):
    """gram -> finish -> update; (return codes, q_out list, kernel [K, K], h, the guarded partials and state)"""
    D = sum(t.shape[1] for t in q)
    slots = lib.raw("zs_svgd_gram_slots", D)
    assert slots == B.slots(D)
    partials, state = ar.out(slots * K * K, F64), ar.out(lib.raw("zs_svgd_state_doubles", K), F64)
    out = q if alias else [ar.out(t.shape, dtype) for t in q]
    tb, n = table(K, q, g, out, h)
    rcs = [lib.raw("zs_svgd_gram" + sfx(dtype), tb, len(q), n, K, ptr(partials), stream()),
           lib.raw("zs_svgd_finish", ptr(partials), slots, K, int(bandwidth is None), bandwidth or 0.0, ptr(state), stream()),
           lib.raw("zs_svgd_update" + sfx(dtype), tb, len(q), n, K, ptr(state), step_size, int(h is not None), int(first), 0.9, 1e-6,
                   stream())]
    return rcs, out, state[B.STATE_HEADER + K:].view(K, K), state[0], (partials, state)


@pytest.fixture(scope="module")
def lib():
    return load("svgd")


def close(name, got, want, tol):
    got = got.cpu().double()
    err = float(((got - want).abs() / torch.as_tensor(tol, dtype=F64)).max())
    print("%s: worst error / tolerance = %.3f" % (name, err))
    assert bool(torch.isfinite(got).all()) and err <= 1.0, "%s: worst error / tolerance %.3f" % (name, err)
    return err


def check_step(lib, dtype, K, thetas, grads, bandwidth, tag, worst=None):
    """one step on both alignments, twice, and aliased; against the truth.  `worst`, a dict, receives the worst error / tolerance
    of the kernel matrix, of h and of the moved particles."""
    worst = {} if worst is None else worst
    t = truth(thetas, grads, bandwidth)
    bphi, bk, bh = bounds(dtype, thetas, grads, t, bandwidth)
    res = []
    for shift in (0, 1):
        ar = Arena(shift)
        q, g = [ar.put(a, dtype) for a in thetas], [ar.put(a, dtype) for a in grads]
        one, again = step(lib, dtype, ar, K, q, g, bandwidth), step(lib, dtype, ar, K, q, g, bandwidth)
        moved = step(lib, dtype, ar, K, [ar.put(a, dtype) for a in thetas], g, bandwidth, alias=True)
        ar.check_guards()
        covered(one[1] + list(one[4]))
        assert one[0] == again[0] == moved[0] == [0, 0, 0]
        for a, b, c in zip(one[1] + [one[2]], again[1] + [again[2]], moved[1] + [moved[2]]):
            assert same_bits(a, b), "the same call twice differs"
            assert same_bits(a, c), "q_out aliasing q_in differs from separate buffers"
        res.append([a.cpu() for a in one[1] + [one[2], one[3]]])
    for a, b in zip(*res):
        assert same_bits(a, b), "the aligned and the shifted layout differ"
    n = len(thetas)
    k = res[0][n]
    assert bool((torch.diagonal(k) == 1).all()) and bool((k == k.t()).all()), "the kernel matrix: unit diagonal, symmetric"
    worst["kernel"] = close("kernel" + tag, k, t[1], bk)
    worst["h"] = close("h" + tag, res[0][n + 1], torch.tensor(t[2], dtype=F64), bh)
    for i in range(n):
        want = thetas[i] + STEP * t[0][i]
        worst["q_out"] = max(worst.get("q_out", 0.0), close("q_out[%d]" % i + tag, res[0][i], want, STEP * bphi + 2 * unit(dtype) * want.abs()))
    return t


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("K,layout,mu", CASES)
def test_values(lib, dtype, K, layout, mu):
    K = K or cap_of(dtype)
    thetas, grads = inputs(K, LAYOUTS[layout], mu)
    check_step(lib, dtype, K, thetas, grads, None, " [K=%d %s mu=%d %s]" % (K, layout, mu, sfx(dtype)))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("what", ["given", "even", "odd", "lattice", "equal"])
def test_bandwidth(lib, dtype, what):
    K = {"given": 9, "even": 6, "odd": 7, "lattice": 12, "equal": 5}[what]
    thetas, grads = inputs(K, [3, 6], 0, seed=5)
    if what == "lattice":          # integer coordinates in {0, 1, 2}: many equal distances, exact in both element types
        thetas = [torch.from_numpy(np.random.default_rng(3).integers(0, 3, (K, m)).astype(np.float64)) for m in (3, 6)]
    if what == "equal":
        thetas = [t[:1].expand(K, -1).contiguous() for t in thetas]
    t = check_step(lib, dtype, K, thetas, grads, 2.5 if what == "given" else None, " [%s %s]" % (what, sfx(dtype)))
    if what == "equal":
        assert t[2] == 1.0 and bool((t[1] == 1).all())          # and phi is the mean gradient, by the truth itself


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
def test_adagrad_two_steps(lib, dtype):
    K, layout, lr = 17, [5, SLAB, 2], 0.5
    thetas, grads = inputs(K, layout, 0, seed=9)
    grads2 = inputs(K, layout, 0, seed=10)[1]
    ar = Arena(1)
    q, g, g2 = ([ar.put(a, dtype) for a in x] for x in (thetas, grads, grads2))
    h = [ar.out(a.shape, dtype) for a in thetas]
    first = step(lib, dtype, ar, K, q, g, h=h, first=True, step_size=lr)
    h1 = [a.cpu().double() for a in h]
    second = step(lib, dtype, ar, K, first[1], g2, h=h, first=False, step_size=lr)
    ar.check_guards()
    assert first[0] == second[0] == [0, 0, 0]
    # With b the bound of phi, s = sqrt H, a = alpha: H = phi^2 moves by 2 |phi| b + b^2, and through the recursion by a times its
    # previous tolerance plus (1 - a) times that.  The direction phi / (fudge + s) moves by at most b / s + |phi| dH / (2 s^3);
    # a phi0^2 <= H and (1 - a) phi^2 <= H give dH <= 2 sqrt 2 b s and |phi| <= s / sqrt(1 - a): (b / s)(1 + sqrt 2 / sqrt(1 - a)) < 6 b / s.
    cur, H, tolH, u = thetas, [None] * len(layout), [0.0] * len(layout), unit(dtype)
    for n, (res, gr, hs) in enumerate(((first, grads, h1), (second, grads2, [a.cpu().double() for a in h]))):
        t = truth(cur, gr)
        bphi = bounds(dtype, cur, gr, t)[0]
        for i, phi in enumerate(t[0]):
            H[i], dirn = precondition(phi, H[i], n == 0, 0.9, 1e-6)
            moved = 2 * phi.abs() * bphi + bphi ** 2
            tolH[i] = moved if n == 0 else 0.9 * tolH[i] + 0.1 * moved
            close("H step %d" % n, hs[i], H[i], tolH[i] + 8 * u * H[i])
            want = cur[i] + lr * dirn
            close("q step %d" % n, res[1][i], want, lr * 6 * bphi / (1e-6 + torch.sqrt(H[i])) + 8 * u * (want.abs() + lr * dirn.abs()))
        cur = [a.cpu().double() for a in res[1]]          # the second step starts where the kernels' first one ended


@pytest.mark.gpu
def test_rejected_calls_write_nothing(lib):
    for dtype in (F32, F64):
        K = 5
        thetas, grads = inputs(K, [3, 4], 0)
        ar = Arena(0)
        q, g = [ar.put(a, dtype) for a in thetas], [ar.put(a, dtype) for a in grads]
        out, partials, state = [ar.out(a.shape, dtype) for a in thetas], ar.out(K * K, F64), ar.out(B.state_doubles(K), F64)
        s, st = sfx(dtype), stream()
        tb, n = table(K, q, g, out)
        gram = lambda tb_, nt, n_, K_, p: lib.raw("zs_svgd_gram" + s, tb_, nt, n_, K_, ptr(p), st)
        upd = lambda tb_, nt, n_, K_, sp, ada=0: lib.raw("zs_svgd_update" + s, tb_, nt, n_, K_, ptr(sp), 1.0, ada, 1, 0.9, 1e-6, st)
        fin = lambda p, sl, K_, med, bw, sp: lib.raw("zs_svgd_finish", ptr(p), sl, K_, med, bw, ptr(sp), st)
        assert gram(None, 2, n, K, partials) == upd(None, 2, n, K, state) == EINVAL
        assert gram(tb, 2, n, 0, partials) == upd(tb, 2, n, 0, state) == fin(partials, 1, 0, 1, 0.0, state) == EINVAL
        assert gram(tb, 2, -1, K, partials) == gram(tb, 0, n, K, partials) == gram(tb, 2, n + 1, K, partials) == EINVAL
        assert gram(tb, 2, n, K, None) == upd(tb, 2, n, K, None) == upd(tb, 2, n, K, state, ada=1) == EINVAL          # (no h in the table)
        assert fin(partials, 1, K, 0, 0.0, state) == fin(partials, 1, K, 0, -1.0, state) == fin(partials, 0, K, 1, 0.0, state) == EINVAL
        assert fin(None, 1, K, 1, 0.0, state) == fin(partials, 1, K, 1, 0.0, None) == EINVAL
        over = cap_of(dtype) + 1
        big, nb = table(over, [ar.put(torch.zeros(over, 1), dtype)])
        assert gram(big, 1, nb, over, partials) == upd(big, 1, nb, over, state) == fin(partials, 1, 257, 1, 0.0, state) == ENOTSUP
        torch.cuda.synchronize()
        assert ar.untouched(), "a rejected call wrote something"
    assert [lib.raw("zs_svgd_max_particles")] + [lib.raw("zs_svgd_max_particles_of", b) for b in (4, 8, 2)] == [256, 256, 128, 0]
    assert [lib.raw("zs_svgd_gram_slots", d) for d in (0, 1, SLAB, SLAB + 1, SLAB * CAP + 1)] == [-1, 1, 1, 2, CAP]
    assert lib.raw("zs_svgd_partial_doubles", 7) == 49 and lib.raw("zs_svgd_partial_doubles", 257) == -1


@pytest.mark.parametrize("K,layout,mu", CASES)
def test_reference_within_its_own_bound(K, layout, mu):
    """CPU: the float32 reference alone is finite and within what its arithmetic allows.  With c the centred particles, a Gram
    entry carries at most (D + 4) u |c_i| |c_j|, so d_ij at most E = 2 (D + 4) u (G_ii + G_jj); the median moves by at most the
    largest E, h in proportion, and k = exp(-d / h) by at most k (E / h) (1 + d / h) <= X = (max E / h) (1 + max d / h); phi is
    a K-term sum of k_ji (g_j + (2/h)(theta_i - theta_j)) / K: (K + 4) u S + 3 X S with S = max|g| + (4/h) max|c|."""
    K = K or 256
    thetas, grads = inputs(K, LAYOUTS[layout], mu)
    t = truth(thetas, grads)
    phis, k, h = torch_step([a.float() for a in thetas], [a.float() for a in grads])
    c = torch.cat(thetas, 1)
    c = c - c.mean(0, keepdim=True)
    D, u, hh = c.shape[1], unit(F32), t[2]
    gmax = float((c ** 2).sum(1).max())
    X = 4 * (D + 4) * u * gmax / hh * (1 + 4 * gmax / hh)
    S = max(float(g.abs().max()) for g in grads) + 4 / hh * float(c.abs().max())
    assert bool(torch.isfinite(k).all()) and all(bool(torch.isfinite(p).all()) for p in phis)
    assert float((k - t[1]).abs().max()) <= X + u
    assert abs(float(h) - hh) <= X * hh + u * hh
    assert max(float((a.double() - b).abs().max()) for a, b in zip(phis, t[0])) <= ((K + 4) * u + 3 * X) * S
