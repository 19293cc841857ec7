"""The flow kernels through the raw C ABI of libzs_flow.so (include/zs_flow.h), on the GPU.

Truth: the header's expression evaluated in numpy long double (x87 extended: 64-bit mantissa) on the same, already rounded
inputs.  Bounds (derived, not measured):

  * an element-wise output: |err| <= 2^-20 S (_f32) or 2^-48 S (_f64), S being the sum of the absolute values of the terms
    that are added for that element -- sixteen roundings of 2^-24 (2^-53) relative each, where the longest expression
    (the masked merge) has seven operations and exp / log / log1p / tanh of the device library are within 2 ulp;
  * a reduction over n terms: |err| <= (n 2^-24 + 2^-20) sum_i S_i (f64: n 2^-53 + 2^-48), S_i the bound's S of term i: the
    first-order error of ANY summation order is at most (n - 1) u sum|t_i|, and each term carries its element-wise error.

Every case runs twice: all operands at aligned addresses (the 4-element path where D % 4 == 0) and all operands shifted by one
element (the element path); both must return the same bits.  Every output lies between NaN guard elements that must stay NaN.
Shapes: B in {1, 3, 65, 257} crosses one wavefront of row lanes and the 16 row lanes of a column tile; D in {1 ... 785} crosses
the 4-element groups, the 64-lane row and the 64-column tile."""
import numpy as np
import pytest
import torch

from kernel_abi import DEV, EINVAL, Arena, load, sfx, stream

pytestmark = pytest.mark.gpu

LD = np.longdouble
NAN = float("nan")          # the fill of every arena of this file
MASK, INTERLEAVE = 0, 1
NORMAL, LOGISTIC = 0, 1
NONE, SCALAR, ROWS = 0, 1, 2
BS = [1, 3, 65, 257]
DS = [1, 2, 3, 4, 5, 8, 63, 64, 65, 257, 785]
DS_PAIRS = [2, 4, 6, 130]
DS_MADE = [1, 3, 4, 65]
DTYPES = [pytest.param(torch.float32, id="f32"), pytest.param(torch.float64, id="f64")]


@pytest.fixture(scope="module")
def lib():
    return load("flow")


def rnd(rng, dtype, *shape):
    """Order-1 values, already rounded to the kernel's dtype (as float64 numpy)."""
    a = rng.standard_normal(shape)
    return torch.from_numpy(a).to(dtype).double().numpy()


def ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def got(t):
    return t.detach().cpu().double().numpy().astype(LD)


def within(g, want, S, dtype, n=None):
    u, e = (2.0 ** -24, 2.0 ** -20) if dtype == torch.float32 else (2.0 ** -53, 2.0 ** -48)
    rel = LD(e if n is None else n * u + e)
    err = np.abs(got(g) - want)
    assert not np.isnan(err).any(), "NaN in the output"
    bad = err > rel * S
    assert not bad.any(), (float(err.max()), float((err / np.maximum(S, LD(1e-300))).max()), float(rel))


def both_offsets(run):
    """run(off) -> list of output tensors; the two layouts must agree bit for bit."""
    a, b = run(0), run(1)
    for x, y in zip(a, b):
        assert torch.equal(x, y), "the aligned and the shifted layout differ"


def mask_for(rng, dtype, D, kind):
    if kind == "binary":
        return (np.arange(D) % 2).astype(np.float64)
    m = rng.choice([0.25, -1.5, 0.0, 1.0], size=D)
    return m.astype(np.float64)


# ------------------------------------------------------------------------------------------------ coupling, MASK
def check_mask(lib, dtype, B, D, maskkind, rng):
    """split, merge and their backwards in MASK mode on one [B, D] problem drawn from `rng`, both signs, both layouts"""
    x, shift, gy = (rnd(rng, dtype, B, D) for _ in range(3))
    mask = mask_for(rng, dtype, D, maskkind)
    X, M, SH, G = ld(x), ld(mask), ld(shift), ld(gy)
    OM = 1 - M
    for sign in (1.0, -1.0):
        def run(off):
            A = Arena(shift=off, fill=NAN, dtype=dtype)
            dx, dm, dsh, dg = A.put(x), A.put(mask), A.put(shift), A.put(gy)
            o_split, o_sbwd, o_y, o_gx, o_gs = (A.out((B, D)) for _ in range(5))
            st = stream()
            assert lib.raw("zs_flow_split" + sfx(dtype), MASK, dx.data_ptr(), dm.data_ptr(), o_split.data_ptr(), B, D, 0, st) == 0
            assert lib.raw("zs_flow_split_bwd" + sfx(dtype), MASK, dg.data_ptr(), dm.data_ptr(), o_sbwd.data_ptr(), B, D, 0, st) == 0
            assert lib.raw("zs_flow_merge" + sfx(dtype), MASK, dx.data_ptr(), dm.data_ptr(), dsh.data_ptr(), sign,
                           o_y.data_ptr(), B, D, 0, st) == 0
            assert lib.raw("zs_flow_merge_bwd" + sfx(dtype), MASK, dg.data_ptr(), dm.data_ptr(), sign, o_gx.data_ptr(),
                           o_gs.data_ptr(), B, D, 0, st) == 0
            A.check_guards()
            within(o_split, M * X, np.abs(M * X), dtype)
            within(o_sbwd, M * G, np.abs(M * G), dtype)
            within(o_y, M * X + (OM * X + sign * SH * OM), np.abs(M * X) + np.abs(OM * X) + np.abs(SH * OM), dtype)
            within(o_gx, M * G + OM * G, np.abs(M * G) + np.abs(OM * G), dtype)
            within(o_gs, sign * G * OM, np.abs(G * OM), dtype)
            return [o_split, o_sbwd, o_y, o_gx, o_gs]
        both_offsets(run)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("maskkind", ["binary", "nonbinary"])
def test_mask_split_merge_and_backwards(lib, dtype, B, maskkind):
    rng = np.random.RandomState(11 + B)
    for D in DS:
        check_mask(lib, dtype, B, D, maskkind, rng)


# ------------------------------------------------------------------------------------------------ coupling, INTERLEAVE
def check_interleave(lib, dtype, B, D, sel, rng):
    """split, merge and their backwards in INTERLEAVE mode on one [B, D] problem drawn from `rng`, both signs, both layouts"""
    on = 1 - sel
    H = D // 2
    x, gy = rnd(rng, dtype, B, D), rnd(rng, dtype, B, D)
    shift, gh = rnd(rng, dtype, B, H), rnd(rng, dtype, B, H)
    X, G, SH = ld(x), ld(gy), ld(shift)
    for sign in (1.0, -1.0):
        def run(off):
            A = Arena(shift=off, fill=NAN, dtype=dtype)
            dx, dg, dsh, dgh = A.put(x), A.put(gy), A.put(shift), A.put(gh)
            o_split, o_gs = A.out((B, H)), A.out((B, H))
            o_sbwd, o_y, o_gx = A.out((B, D)), A.out((B, D)), A.out((B, D))
            st = stream()
            assert lib.raw("zs_flow_split" + sfx(dtype), INTERLEAVE, dx.data_ptr(), None, o_split.data_ptr(), B, D, sel, st) == 0
            assert lib.raw("zs_flow_split_bwd" + sfx(dtype), INTERLEAVE, dgh.data_ptr(), None, o_sbwd.data_ptr(), B, D, sel, st) == 0
            assert lib.raw("zs_flow_merge" + sfx(dtype), INTERLEAVE, dx.data_ptr(), None, dsh.data_ptr(), sign, o_y.data_ptr(),
                           B, D, sel, st) == 0
            assert lib.raw("zs_flow_merge_bwd" + sfx(dtype), INTERLEAVE, dg.data_ptr(), None, sign, o_gx.data_ptr(),
                           o_gs.data_ptr(), B, D, sel, st) == 0
            A.check_guards()
            assert torch.equal(o_split, dx[:, sel::2])                                  # copies are exact
            assert torch.equal(o_sbwd[:, sel::2], dgh) and bool((o_sbwd[:, on::2] == 0).all())
            assert torch.equal(o_y[:, sel::2], dx[:, sel::2])
            within(o_y[:, on::2], X[:, on::2] + sign * SH, np.abs(X[:, on::2]) + np.abs(SH), dtype)
            assert torch.equal(o_gx, dg)
            assert torch.equal(o_gs, sign * dg[:, on::2])
            return [o_split, o_sbwd, o_y, o_gx, o_gs]
        both_offsets(run)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("sel", [0, 1])
def test_interleave_split_merge_and_backwards(lib, dtype, B, sel):
    rng = np.random.RandomState(23 + B + sel)
    for D in DS_PAIRS:
        check_interleave(lib, dtype, B, D, sel, rng)


# ------------------------------------------------------------------------------------------------ Scaling
def check_scale(lib, dtype, B, D, rng):
    """Scaling forward (out of place and in place) and backward on one [B, D] problem drawn from `rng`, both signs, both layouts"""
    x, gy, ls, gld = rnd(rng, dtype, B, D), rnd(rng, dtype, B, D), rnd(rng, dtype, D), rnd(rng, dtype, 1)
    X, G, LS = ld(x), ld(gy), ld(ls)
    for sign in (1.0, -1.0):
        F = np.exp(sign * LS)
        Y = X * F

        def run(off):
            A = Arena(shift=off, fill=NAN, dtype=dtype)
            dx, dg, dls, dgl = A.put(x), A.put(gy), A.put(ls), A.put(gld)
            o_y, o_ld, o_gx, o_gls, o_gls0 = A.out((B, D)), A.out(1), A.out((B, D)), A.out(D), A.out(D)
            inplace = A.put(x)
            o_ld2, o_gls2 = A.out(1), A.out(D)
            st = stream()
            name = "zs_flow_scale_fwd" + sfx(dtype)
            assert lib.raw(name, dx.data_ptr(), dls.data_ptr(), sign, o_y.data_ptr(), o_ld.data_ptr(), B, D, st) == 0
            assert lib.raw(name, inplace.data_ptr(), dls.data_ptr(), sign, inplace.data_ptr(), o_ld2.data_ptr(), B, D, st) == 0
            name = "zs_flow_scale_bwd" + sfx(dtype)
            args = (dg.data_ptr(), o_y.data_ptr(), dls.data_ptr())
            assert lib.raw(name, *args, dgl.data_ptr(), sign, o_gx.data_ptr(), o_gls.data_ptr(), B, D, st) == 0
            assert lib.raw(name, *args, dgl.data_ptr(), sign, o_gx.data_ptr(), o_gls2.data_ptr(), B, D, st) == 0
            assert lib.raw(name, *args, None, sign, o_gx.data_ptr(), o_gls0.data_ptr(), B, D, st) == 0
            A.check_guards()
            within(o_y, Y, np.abs(Y), dtype)
            assert torch.equal(inplace, o_y), "in place differs from out of place"
            within(o_ld, LS.sum(), np.abs(LS).sum(), dtype, n=D)
            assert torch.equal(o_ld, o_ld2) and torch.equal(o_gls, o_gls2), "a reduction is not reproducible"
            within(o_gx, G * F, np.abs(G * F), dtype)
            Yk = got(o_y)                      # the backward reads the SAVED output: the truth uses the same numbers
            S = np.abs(G * Yk).sum(0)
            within(o_gls, sign * (G * Yk).sum(0) + ld(gld)[0], S + abs(ld(gld)[0]), dtype, n=B + 1)
            within(o_gls0, sign * (G * Yk).sum(0), S, dtype, n=B)
            return [o_y, o_ld, o_gx, o_gls, o_gls0]
        both_offsets(run)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", BS)
def test_scale_forward_and_backward(lib, dtype, B):
    rng = np.random.RandomState(37 + B)
    for D in DS:
        check_scale(lib, dtype, B, D, rng)


# ------------------------------------------------------------------------------------------------ MADE's affine
def check_made(lib, dtype, B, D, rng):
    """MADE's affine forward, backward and inverse column on one [B, D] problem drawn from `rng`, both layouts"""
    x, gu, gld, net = rnd(rng, dtype, B, D), rnd(rng, dtype, B, D), rnd(rng, dtype, B, D), rnd(rng, dtype, B, 2 * D)
    X, GU, GL, NET = ld(x), ld(gu), ld(gld), ld(net)
    Mn, LA = NET[:, :D], NET[:, D:]
    E = np.exp(-LA)
    U = (X - Mn) * E
    Su = (np.abs(X) + np.abs(Mn)) * E
    col = D // 2

    def run(off):
        A = Arena(shift=off, fill=NAN, dtype=dtype)
        dx, dgu, dgl, dnet = A.put(x), A.put(gu), A.put(gld), A.put(net)
        o_u, o_ld, o_gx, o_gx2, o_inv = (A.out((B, D)) for _ in range(5))
        o_gnet, o_gnet2 = A.out((B, 2 * D)), A.out((B, 2 * D))
        o_inv.fill_(7.0)
        st = stream()
        assert lib.raw("zs_flow_made_fwd" + sfx(dtype), dx.data_ptr(), dnet.data_ptr(), o_u.data_ptr(), o_ld.data_ptr(), B, D, st) == 0
        assert lib.raw("zs_flow_made_bwd" + sfx(dtype), dgu.data_ptr(), dgl.data_ptr(), dx.data_ptr(), dnet.data_ptr(),
                       o_gx.data_ptr(), o_gnet.data_ptr(), B, D, st) == 0
        assert lib.raw("zs_flow_made_bwd" + sfx(dtype), dgu.data_ptr(), None, dx.data_ptr(), dnet.data_ptr(),
                       o_gx2.data_ptr(), o_gnet2.data_ptr(), B, D, st) == 0
        assert lib.raw("zs_flow_made_inv_col" + sfx(dtype), dgu.data_ptr(), dnet.data_ptr(), o_inv.data_ptr(), B, D, col, st) == 0
        A.check_guards()
        within(o_u, U, Su, dtype)
        assert torch.equal(o_ld, -dnet[:, D:])
        within(o_gx, GU * E, np.abs(GU * E), dtype)
        within(o_gnet[:, :D], -GU * E, np.abs(GU * E), dtype)
        within(o_gnet[:, D:], -(GU * U) - GL, np.abs(GU) * Su + np.abs(GL), dtype)
        assert torch.equal(o_gx, o_gx2) and torch.equal(o_gnet[:, :D], o_gnet2[:, :D])
        within(o_gnet2[:, D:], -(GU * U), np.abs(GU) * Su, dtype)
        inv = GU[:, col] * np.exp(LA[:, col]) + Mn[:, col]
        within(o_inv[:, col], inv, np.abs(GU[:, col] * np.exp(LA[:, col])) + np.abs(Mn[:, col]), dtype)
        others = [c for c in range(D) if c != col]
        assert bool((o_inv[:, others] == 7.0).all()), "another column was written"
        return [o_u, o_ld, o_gx, o_gnet, o_inv]
    both_offsets(run)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", BS)
def test_made_affine_forward_backward_and_inverse_column(lib, dtype, B):
    rng = np.random.RandomState(41 + B)
    for D in DS_MADE:
        check_made(lib, dtype, B, D, rng)


# ------------------------------------------------------------------------------------------------ FlowDistribution tail
def base_truth(base, Z, LOC, SC):
    """(lp, S of lp, d lp / dz) in long double."""
    if base == NORMAL:
        c = LD(-0.91893853320467274178)
        prec = 1 / (SC * SC)
        q = LD(0.5) * prec * (Z - LOC) ** 2
        return (c - np.log(SC)) - q, np.abs(c) + np.abs(np.log(SC)) + q, -(prec * (Z - LOC))
    t = (Z - LOC) / SC
    at = np.abs(t)
    sp = 2 * np.log1p(np.exp(-at))
    return -(at + sp) - np.log(SC), at + sp + np.abs(np.log(SC)), -(np.tanh(t / 2) / SC)


def check_tail(lib, dtype, B, D, base, rng):
    """The tail's forward (three logdet kinds) and backward on one [B, D] problem drawn from `rng`, parameters per column and
    per element, both layouts"""
    for param_rows in (0, 1):
        pshape = (B, D) if param_rows else (D,)
        z, g = rnd(rng, dtype, B, D), rnd(rng, dtype, B)
        loc = rnd(rng, dtype, *pshape)
        scale = torch.from_numpy(np.exp(0.5 * rng.standard_normal(pshape))).to(dtype).double().numpy()
        lds, ldr = rnd(rng, dtype, 1), rnd(rng, dtype, B)
        Z, G, LOC, SC = ld(z), ld(g), ld(loc), ld(scale)
        lp, S, dz = base_truth(base, Z, LOC, SC)

        def run(off):
            A = Arena(shift=off, fill=NAN, dtype=dtype)
            dz_, dg, dloc, dsc, dlds, dldr = A.put(z), A.put(g), A.put(loc), A.put(scale), A.put(lds), A.put(ldr)
            o_n, o_s, o_r, o_r2, o_gl = (A.out(B) for _ in range(5))
            o_gz, o_gz2 = A.out((B, D)), A.out((B, D))
            st = stream()
            name = "zs_flow_tail" + sfx(dtype)
            head = (base, dz_.data_ptr(), dloc.data_ptr(), dsc.data_ptr(), param_rows)
            assert lib.raw(name, *head, None, NONE, o_n.data_ptr(), B, D, st) == 0
            assert lib.raw(name, *head, dlds.data_ptr(), SCALAR, o_s.data_ptr(), B, D, st) == 0
            assert lib.raw(name, *head, dldr.data_ptr(), ROWS, o_r.data_ptr(), B, D, st) == 0
            assert lib.raw(name, *head, dldr.data_ptr(), ROWS, o_r2.data_ptr(), B, D, st) == 0
            name = "zs_flow_tail_bwd" + sfx(dtype)
            head = (base, dg.data_ptr(), dz_.data_ptr(), dloc.data_ptr(), dsc.data_ptr(), param_rows)
            assert lib.raw(name, *head, o_gz.data_ptr(), o_gl.data_ptr(), B, D, st) == 0
            assert lib.raw(name, *head, o_gz2.data_ptr(), None, B, D, st) == 0
            A.check_guards()
            within(o_n, lp.sum(1), S.sum(1), dtype, n=D)
            within(o_s, lp.sum(1) + ld(lds)[0], S.sum(1) + abs(ld(lds)[0]), dtype, n=D + 1)
            within(o_r, lp.sum(1) + ld(ldr), S.sum(1) + np.abs(ld(ldr)), dtype, n=D + 1)
            assert torch.equal(o_r, o_r2), "the row reduction is not reproducible"
            within(o_gz, G[:, None] * dz, np.abs(G[:, None] * dz), dtype)
            assert torch.equal(o_gz, o_gz2) and torch.equal(o_gl, dg)
            return [o_n, o_s, o_r, o_gz, o_gl]
        both_offsets(run)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("base", [NORMAL, LOGISTIC], ids=["normal", "logistic"])
def test_tail_forward_and_backward(lib, dtype, B, base):
    rng = np.random.RandomState(53 + B + base)
    for D in DS:
        check_tail(lib, dtype, B, D, base, rng)


# ------------------------------------------------------------------------------------------------ edges
def _calls(t, B, D, dtype):
    """Every entry with valid operands of a [B, D] problem: (name, args without the stream).  `t` supplies pointers."""
    p = t.data_ptr()
    s = sfx(dtype)
    return [
        ("zs_flow_split" + s, (MASK, p, p, p, B, D, 0)),
        ("zs_flow_split" + s, (INTERLEAVE, p, None, p, B, D, 1)),
        ("zs_flow_split_bwd" + s, (MASK, p, p, p, B, D, 0)),
        ("zs_flow_split_bwd" + s, (INTERLEAVE, p, None, p, B, D, 0)),
        ("zs_flow_merge" + s, (MASK, p, p, p, 1.0, p, B, D, 0)),
        ("zs_flow_merge" + s, (INTERLEAVE, p, None, p, 1.0, p, B, D, 0)),
        ("zs_flow_merge_bwd" + s, (MASK, p, p, -1.0, p, p, B, D, 0)),
        ("zs_flow_merge_bwd" + s, (INTERLEAVE, p, None, -1.0, p, p, B, D, 1)),
        ("zs_flow_scale_fwd" + s, (p, p, 1.0, p, p, B, D)),
        ("zs_flow_scale_bwd" + s, (p, p, p, p, 1.0, p, p, B, D)),
        ("zs_flow_made_fwd" + s, (p, p, p, p, B, D)),
        ("zs_flow_made_bwd" + s, (p, p, p, p, p, p, B, D)),
        ("zs_flow_made_inv_col" + s, (p, p, p, B, D, 0)),
        ("zs_flow_tail" + s, (NORMAL, p, p, p, 0, p, ROWS, p, B, D)),
        ("zs_flow_tail_bwd" + s, (LOGISTIC, p, p, p, p, 1, p, p, B, D)),
    ]


@pytest.mark.parametrize("dtype", DTYPES)
def test_empty_problems_launch_nothing(lib, dtype):
    t = torch.full((64,), 5.0, dtype=dtype, device=DEV)
    st = stream()
    for B, D in [(0, 4), (4, 0), (0, 0)]:
        for name, args in _calls(t, B, D, dtype):
            assert lib.raw(name, *args, st) == 0, (name, B, D)
    torch.cuda.synchronize()
    assert bool((t == 5.0).all()), "an empty problem wrote something"


@pytest.mark.parametrize("dtype", DTYPES)
def test_rejected_arguments_return_their_code_without_a_launch(lib, dtype):
    t = torch.full((64,), 5.0, dtype=dtype, device=DEV)
    p, s, st = t.data_ptr(), sfx(dtype), stream()
    B, D = 2, 4
    for name, args in _calls(t, B, D, dtype):
        ib = len(args) - 2 - (1 if "split" in name or "merge" in name or "inv_col" in name else 0)          # where B sits
        for bad_b, bad_d in [(-1, D), (B, -1)]:
            a = list(args)
            a[ib], a[ib + 1] = bad_b, bad_d
            assert lib.raw(name, *a, st) == EINVAL, (name, "negative size")
        # every pointer in turn replaced by NULL: rejected unless the header makes that operand optional
        optional = {"zs_flow_scale_bwd": [3], "zs_flow_made_bwd": [0, 1], "zs_flow_tail_bwd": [7]}.get(name[:-4], [])
        if args[0] == INTERLEAVE and ("split" in name or "merge" in name):
            optional = [2]                                                    # the mask of INTERLEAVE mode
        for i, v in enumerate(args):
            if v == p and i not in optional:
                a = list(args)
                a[i] = None
                assert lib.raw(name, *a, st) == EINVAL, (name, "NULL argument %d" % i)
    # odd D and a bad sel in INTERLEAVE mode; unknown mode / base / kind; column out of range; both MADE gradients absent
    assert lib.raw("zs_flow_split" + s, INTERLEAVE, p, None, p, B, 5, 0, st) == EINVAL
    assert lib.raw("zs_flow_split_bwd" + s, INTERLEAVE, p, None, p, B, 5, 0, st) == EINVAL
    assert lib.raw("zs_flow_merge" + s, INTERLEAVE, p, None, p, 1.0, p, B, 5, 0, st) == EINVAL
    assert lib.raw("zs_flow_merge_bwd" + s, INTERLEAVE, p, None, 1.0, p, p, B, 5, 0, st) == EINVAL
    assert lib.raw("zs_flow_split" + s, INTERLEAVE, p, None, p, B, D, 2, st) == EINVAL
    assert lib.raw("zs_flow_merge" + s, INTERLEAVE, p, None, p, 1.0, p, B, D, -1, st) == EINVAL
    assert lib.raw("zs_flow_split" + s, 2, p, p, p, B, D, 0, st) == EINVAL
    assert lib.raw("zs_flow_merge" + s, 7, p, p, p, 1.0, p, B, D, 0, st) == EINVAL
    assert lib.raw("zs_flow_tail" + s, 2, p, p, p, 0, p, ROWS, p, B, D, st) == EINVAL
    assert lib.raw("zs_flow_tail" + s, NORMAL, p, p, p, 2, p, ROWS, p, B, D, st) == EINVAL
    assert lib.raw("zs_flow_tail" + s, NORMAL, p, p, p, 0, p, 3, p, B, D, st) == EINVAL
    assert lib.raw("zs_flow_tail" + s, NORMAL, p, p, p, 0, None, SCALAR, p, B, D, st) == EINVAL
    assert lib.raw("zs_flow_tail_bwd" + s, -1, p, p, p, p, 0, p, None, B, D, st) == EINVAL
    assert lib.raw("zs_flow_made_inv_col" + s, p, p, p, B, D, D, st) == EINVAL
    assert lib.raw("zs_flow_made_inv_col" + s, p, p, p, B, D, -1, st) == EINVAL
    assert lib.raw("zs_flow_made_bwd" + s, None, None, p, p, p, p, B, D, st) == EINVAL
    torch.cuda.synchronize()
    assert bool((t == 5.0).all()), "a rejected call wrote something"
    assert lib.cdll.zs_flow_abi_version() == 1
