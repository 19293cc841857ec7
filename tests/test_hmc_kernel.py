"""The HMC kernels through the raw C ABI of libzs_hmc.so (include/zs_hmc.h), on the GPU.

Truth: a float64 torch evaluation of the header's formulas on the same inputs.  Bounds, as tests/test_mcmc_kernel.py: an
element is held to |err| <= 2^-20 S for _f32 (2^-48 S for _f64), S the sum of the absolute values of the terms added; a
kinetic sum over n terms to (n 2^-24 + 2^-20) sum_i S_i (n 2^-53 + 2^-48 for _f64), S_i the bound's S of term i.  Every layout
runs with aligned operands (the 16-byte path where starts and rows allow it) and with every operand shifted by one element
(the element path): the two must agree bit for bit, and sentinel elements around every output must survive."""
import ctypes

import numpy as np
import pytest
import torch

import hmc_host
from kernel_abi import DEV, EINVAL, ENOTSUP, F32, F64, SENTINEL, Arena, load, ptr, sfx, stream

pytestmark = pytest.mark.gpu

BEGIN, STEP, END = 0, 1, 2
EPS = 0.37


@pytest.fixture(scope="module")
def lib():
    return load("hmc")


def state_block(eps=EPS, **kw):
    s = [eps, eps, 0., 0., 0., 0., 0., 0.]
    for k, v in kw.items():
        s[getattr(hmc_host, k)] = v
    return torch.tensor(s, dtype=F64, device=DEV)


def raw_move(lib, dtype, kind, rows, n, C, state, ksum, seed=0, call=0, rs=None, n_tensors=None):
    """rows: dicts with q0, q, p, grad, z, p0, start, row (tensors, None, or raw addresses); returns the entry point's code."""
    from zhusuan import _hmc_hip
    table = (_hmc_hip.HmcTensor * max(len(rows), 1))()
    for e, r in zip(table, rows):
        for k in ("q0", "q", "p", "grad", "z", "p0", "q_out"):
            setattr(e, k, ptr(r.get(k)))
        e.start, e.row = r["start"], r["row"]
    return lib.raw("zs_hmc_move" + sfx(dtype), kind, table if rows else None, len(rows) if n_tensors is None else n_tensors, n, C,
                   ptr(state), ptr(ksum), seed, call, ptr(rs), stream())


def raw_select(lib, dtype, rows, n, C, accept, n_tensors=None):
    from zhusuan import _hmc_hip
    table = (_hmc_hip.HmcTensor * max(len(rows), 1))()
    for e, r in zip(table, rows):
        for k in ("q0", "q", "q_out"):
            setattr(e, k, ptr(r.get(k)))
        e.start, e.row = r["start"], r["row"]
    return lib.raw("zs_hmc_select" + sfx(dtype), table if rows else None, len(rows) if n_tensors is None else n_tensors, n, C,
                   ptr(accept), stream())


def raw_decide(lib, dtype, chunks, C, logp0, logp1, u, state, out, accept, adapting=0, delta=0.8, gamma=0.05, t0=100., kappa=0.75,
               seed=0, call=0, rs=None, n_chunks=None):
    from zhusuan import _hmc_hip
    table = (_hmc_hip.HmcChunk * max(len(chunks), 1))()
    for e, (k0, k1, slots, f64) in zip(table, chunks):
        e.k0, e.k1, e.slots, e.is_f64 = ptr(k0), ptr(k1), slots, f64
    return lib.raw("zs_hmc_decide" + sfx(dtype), table if chunks else None, len(chunks) if n_chunks is None else n_chunks, C,
                   ptr(logp0), ptr(logp1), ptr(u), ptr(state), ptr(out), ptr(accept), adapting, delta, gamma, t0, kappa,
                   seed, call, ptr(rs), stream())


def place(ar, flat, sizes):
    """Device copies of the pieces of `flat`, each inside a guarded buffer of its own in the arena `ar`; returns the views."""
    return [ar.put(piece) for piece in torch.split(flat, sizes)]


def cat(views):
    return torch.cat([v.cpu() for v in views])


def inputs(n, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=gen, dtype=F64).to(dtype) for _ in range(4)]          # q, p, g, z


def run_move(lib, dtype, kind, C, rows, shift, data, inject=True, seed=5, call=9, rs=None, eps=EPS):
    """One move on tensors laid out as (C, rows) with every operand shifted by `shift` elements; returns host tensors
    (q, p, p0, ksum[C, slots]) -- None where the kind does not write them."""
    q, p, g, z = data
    sizes = [C * r for r in rows]
    starts = [int(x) for x in np.cumsum([0] + sizes)]
    n = starts[-1]
    slots = sum(hmc_host.pieces(r) for r in rows)
    zero = torch.zeros_like(q)
    ar = Arena(shift)
    vq0 = place(ar, q, sizes)
    vq = place(ar, zero if kind == BEGIN else q, sizes)
    vp = place(ar, zero if kind == BEGIN else p, sizes)
    vg = place(ar, g, sizes)
    vz = place(ar, z, sizes)
    vp0 = place(ar, zero, sizes)
    ks = place(ar, torch.full((C * slots,), float("nan"), dtype=dtype), [C * slots])
    table = [dict(q0=vq0[i], q=vq[i], p=vp[i], grad=vg[i], z=vz[i] if inject else None, p0=vp0[i], start=starts[i], row=rows[i])
             for i in range(len(rows))]
    rc = raw_move(lib, dtype, kind, table, n, C, state_block(eps), ks[0], seed=seed, call=call, rs=rs)
    assert rc == 0, rc
    ar.check_guards()
    assert torch.equal(cat(vq0), q) and torch.equal(cat(vg), g) and torch.equal(cat(vz), z), "an input was modified"
    ksum = ks[0].cpu().view(C, slots)
    if kind == STEP:
        assert bool(torch.isnan(ksum).all()), "STEP wrote to the workspace"
        return cat(vq), cat(vp), None, None
    assert not bool(torch.isnan(ksum).any()), "a slot of the workspace was not written"
    if kind == BEGIN:
        return cat(vq), cat(vp), cat(vp0), ksum
    assert torch.equal(cat(vp), p), "END modified p"
    return None, None, None, ksum


def rel(dtype):
    return 2.0 ** -20 if dtype == F32 else 2.0 ** -48


def within(got, want, S, dtype):
    err = (got.double() - want).abs()
    bad = err > rel(dtype) * S
    assert not bool(bad.any()), (float(err.max()), float((err / S.clamp_min(1e-300)).max()), rel(dtype))


def per_chain(flat, C, rows):
    """Sum over every tensor's row of chain c of a flat [n] float64 tensor -> [C]."""
    out, a = torch.zeros(C, dtype=F64), 0
    for r in rows:
        out += flat[a:a + C * r].view(C, r).sum(dim=1)
        a += C * r
    return out


def check_kinetic(ksum, terms, S, C, rows, dtype):
    n = sum(rows)
    ulp = 2.0 ** -24 if dtype == F32 else 2.0 ** -53
    got = 0.5 * ksum.double().sum(dim=1)
    want = 0.5 * per_chain(terms, C, rows)
    bound = (n * ulp + rel(dtype)) * 0.5 * per_chain(S, C, rows)
    err = (got - want).abs()
    assert bool((err <= bound).all()), (float(err.max()), float((err / bound.clamp_min(1e-300)).max()))


def check_kind(lib, dtype, kind, C, rows, seed, shifts=(0, 1)):
    n = C * sum(rows)
    q, p, g, z = data = inputs(n, dtype, seed)
    g[::5] = 0.0
    p[::7] = 0.0
    e, h = EPS, 0.5 * EPS
    Q, P, G, Z = [t.double() for t in data]
    outs = [run_move(lib, dtype, kind, C, rows, s, data) for s in shifts]
    again = run_move(lib, dtype, kind, C, rows, shifts[0], data)
    for o in outs[1:] + [again]:
        for a, b in zip(outs[0], o):
            assert (a is None and b is None) or torch.equal(a, b), "layouts or runs differ in bits"
    q2, p2, p02, ksum = outs[0]
    if kind == BEGIN:
        Sp = Z.abs() + (h * G).abs()
        within(p2, Z + h * G, Sp, dtype)
        within(q2, Q + e * (Z + h * G), Q.abs() + e * Sp, dtype)
        assert torch.equal(p02, z)
        check_kinetic(ksum, Z * Z, Z * Z, C, rows, dtype)
    elif kind == STEP:
        Sp = P.abs() + (e * G).abs()
        within(p2, P + e * G, Sp, dtype)
        within(q2, Q + e * (P + e * G), Q.abs() + e * Sp, dtype)
    else:
        Sp = P.abs() + (h * G).abs()
        check_kinetic(ksum, (P + h * G) ** 2, Sp * Sp, C, rows, dtype)
    return data, outs[0]


# ------------------------------------------------------------------------------------------------ 1. moves
SHAPES = sorted(set([(C, r) for C in (1, 3, 64, 65, 257) for r in (1, 5, 64)] +
                    [(C, r) for r in (1, 3, 4, 5, 63, 64, 65, 257, 4099) for C in (1, 3)]))


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("C,row", SHAPES, ids=["C%dxrow%d" % s for s in SHAPES])
def test_every_kind_matches_the_float64_formulas(lib, C, row, dtype):
    for kind in (BEGIN, STEP, END):
        check_kind(lib, dtype, kind, C, [row], 100 * C + row + kind)


MULTI = [("5+7", 3, [5, 7]), ("8+12", 3, [8, 12]), ("32x4", 3, [4] * 32), ("tile_edges", 2, [1023, 1025, 2, 2047]),
         ("8+12_one_chain", 1, [8, 12])]


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("name,C,rows", MULTI, ids=[m[0] for m in MULTI])
def test_several_tensors_with_different_rows(lib, name, C, rows, dtype):
    for kind in (BEGIN, STEP, END):
        check_kind(lib, dtype, kind, C, rows, 7 + kind)


def test_one_chain_across_many_workgroups(lib):
    """C = 1 with 2^20 + 5 elements: 1025 tiles, one slot each."""
    for kind in (BEGIN, END):
        check_kind(lib, F32, kind, 1, [(1 << 20) + 5], 11 + kind)


def test_an_offset_view_among_aligned_tensors(lib):
    """One tensor of three starts one element into its buffer: the whole launch takes the element path, with the aligned bits."""
    C, rows = 3, [8, 16, 4]
    data = inputs(C * sum(rows), F32, 3)
    a = run_move(lib, F32, BEGIN, C, rows, 0, data)
    q, p, g, z = data
    sizes = [C * r for r in rows]
    starts = [0, sizes[0], sizes[0] + sizes[1]]
    ops = {}
    for name, flat in (("q0", q), ("q", torch.zeros_like(q)), ("p", torch.zeros_like(q)), ("grad", g), ("z", z), ("p0", torch.zeros_like(q))):
        ops[name] = [Arena(1 if i == 1 and name in ("q", "grad") else 0).put(flat[s:s + k]) for i, (s, k) in enumerate(zip(starts, sizes))]
    slots = sum(hmc_host.pieces(r) for r in rows)
    ks = torch.full((C * slots,), float("nan"), device=DEV)
    table = [dict(dict((k, v[i]) for k, v in ops.items()), start=starts[i], row=rows[i]) for i in range(3)]
    assert raw_move(lib, F32, BEGIN, table, sum(sizes), C, state_block(), ks) == 0
    torch.cuda.synchronize()
    assert torch.equal(cat(ops["q"]), a[0]) and torch.equal(cat(ops["p"]), a[1]) and torch.equal(ks.cpu().view(C, slots), a[3])


# ------------------------------------------------------------------------------------------------ 2. stream
def philox(name, n, seed, call, rs=None):
    """Elements [0, n) of the MAIN library's stream."""
    from zhusuan import _hip
    out = torch.empty(n, dtype=F32, device=DEV)
    _hip.lib().call(name, out.data_ptr(), n, seed, call, ptr(rs), _hip.stream_for(out))
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("C,rows,shift", [(1, [5, 7], 0), (1, [8, 12], 0), (3, [8, 12], 1), (65, [64], 0)],
                         ids=["element", "vector", "shifted", "many_tiles"])
def test_drawn_momentum_is_the_main_librarys_philox_stream(lib, C, rows, shift, dtype):
    n = C * sum(rows)
    q, p, g, _ = inputs(n, dtype, 7)
    zero = torch.zeros(n, dtype=dtype)
    seed, call = 0x1234ABCD5678, 41
    rs = torch.tensor([99, 1 << 20], dtype=torch.int64, device=DEV)          # {seed, non-zero base}
    first = None
    for kw, stream_args in [(dict(seed=seed, call=call), (seed, call, None)), (dict(seed=1, call=3, rs=rs), (1, 3, rs)),
                            (dict(seed=seed, call=call + 1), (seed, call + 1, None))]:
        drawn = run_move(lib, dtype, BEGIN, C, rows, shift, (q, p, g, zero), inject=False, **kw)
        z = philox("zs_philox_normal_f32", n, *stream_args).to(dtype)
        given = run_move(lib, dtype, BEGIN, C, rows, shift, (q, p, g, z), inject=True, seed=0, call=0)
        assert all(torch.equal(a, b) for a, b in zip(drawn, given))
        assert torch.equal(drawn[2], z)
        if first is None:
            first = drawn
    assert not torch.equal(first[2], drawn[2]), "call + 1 drew the same noise"


# ------------------------------------------------------------------------------------------------ 3. decide
DECIDE_SEEDS = {1: 1, 3: 1, 65: 1, 257: 1}


def decide_inputs(C, seed):
    """Two chunks (float32 with 3 slots, float64 with 2), log joints and uniforms of C chains; host tensors."""
    gen = torch.Generator().manual_seed(seed)

    def rnd(*s):
        return torch.randn(*s, generator=gen, dtype=F64)
    k = [(rnd(C, 3) ** 2).float(), (rnd(C, 3) ** 2).float(), rnd(C, 2) ** 2, rnd(C, 2) ** 2]
    l0, l1 = -3.0 + rnd(C), -3.0 + rnd(C)
    u = torch.rand(C, generator=gen, dtype=F64).clamp_min(1e-6)
    return k, l0, l1, u


def decide_truth(k, l0, l1, u, state, adapting):
    k0 = 0.5 * (k[0].double().sum(dim=1) + k[2].sum(dim=1))
    k1 = 0.5 * (k[1].double().sum(dim=1) + k[3].sum(dim=1))
    acc, a, dh, st = hmc_host.decide_math(k0, k1, l0.double(), l1.double(), u.double(), state, adapting, 0.8, 0.05, 100., 0.75)
    return dict(acc=acc, a=a, dh=dh, st=st, h0=k0 - l0.double(), h1=k1 - l1.double(), S=l0.abs().double() + l1.abs().double() + k0 + k1)


def guarded(t, u):
    """Chains whose decision the float64 restatement cannot vouch for: log u within 1e-3 (1 + |dH|) of dH."""
    dh = t["dh"]
    return torch.isfinite(dh) & ((torch.log(u.double()) - dh).abs() <= 1e-3 * (1.0 + dh.abs()))


def run_decide(lib, dtype, C, k, l0, l1, u, state, adapting=0, seed=0, call=0, rs=None):
    d = [t.to(DEV) for t in k]
    L0, L1 = l0.to(dtype).to(DEV), l1.to(dtype).to(DEV)
    U = None if u is None else u.to(dtype).to(DEV)
    ar = Arena()
    out, acc = ar.out((5, C), F64), ar.out(C, torch.int32)
    rc = raw_decide(lib, dtype, [(d[0], d[1], 3, 0), (d[2], d[3], 2, 1)], C, L0, L1, U, state, out, acc,
                    adapting=adapting, seed=seed, call=call, rs=rs)
    assert rc == 0, rc
    ar.check_guards()
    return out.cpu(), acc.cpu(), state.cpu()


def close40(got, want, scale=None):
    scale = want.abs() if scale is None else scale
    err = (got - want).abs()
    assert bool((err <= 2.0 ** -40 * scale + 1e-300).all()), float((err / scale.clamp_min(1e-300)).max())


def check_decide(lib, dtype, C, seed):
    """One adapting decide of C chains on decide_inputs(C, seed) against the float64 restatement: all five `out` rows, `accept`
    outside the guard, and the whole state block (step size, averages, ABAR, NACC); returns (k, l0, l1, u, t, out, acc, st)."""
    k, l0, l1, u = decide_inputs(C, seed)
    l0, l1, u = [t.to(dtype) for t in (l0, l1, u)]          # what the kernel is given
    st0 = [EPS, EPS, 0., 0., 0., 0., 0., 0.]
    t = decide_truth(k, l0, l1, u, st0, True)
    left_out = guarded(t, u)
    assert int(left_out.sum()) <= 0.02 * C, "the fixed seed leaves too many chains to the guard"
    out, acc, st = run_decide(lib, dtype, C, k, l0, l1, u, state_block(), adapting=1)
    close40(out[3], t["dh"], t["S"])
    close40(out[0], t["a"])
    close40(out[1], t["h0"], t["S"])
    close40(out[2], t["h1"], t["S"])
    ok = ~left_out
    assert torch.equal(acc.bool()[ok], t["acc"][ok])
    assert torch.equal(out[4], torch.where(acc.bool(), l1.double(), l0.double()))
    close40(st[:7], torch.tensor(t["st"][:7], dtype=F64), torch.tensor([1 + abs(x) for x in t["st"][:7]], dtype=F64))
    assert float(st[7]) == float(acc.sum())
    return k, l0, l1, u, t, out, acc, st


@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("C", [1, 3, 65, 257])
def test_decide_matches_the_double_restatement_and_isolates_non_finite_chains(lib, C, dtype):
    k, l0, l1, u, t, out, acc, st = check_decide(lib, dtype, C, DECIDE_SEEDS[C])
    # a second adapting decide, then a frozen one, on the block the first one left
    dev_state = st.to(DEV)
    _, _, st2 = run_decide(lib, dtype, C, k, l0, l1, u, dev_state, adapting=1)
    t2 = decide_truth(k, l0, l1, u, t["st"], True)
    close40(st2[:7], torch.tensor(t2["st"][:7], dtype=F64), torch.tensor([1 + abs(x) for x in t2["st"][:7]], dtype=F64))
    _, _, st3 = run_decide(lib, dtype, C, k, l0, l1, u, dev_state, adapting=0)
    t3 = decide_truth(k, l0, l1, u, t2["st"], False)
    close40(st3[:7], torch.tensor(t3["st"][:7], dtype=F64), torch.tensor([1 + abs(x) for x in t3["st"][:7]], dtype=F64))
    assert float(st3[0]) == float(torch.exp(st3[5])) or abs(float(st3[0]) - float(torch.exp(st3[5]))) <= 2.0 ** -40 * float(st3[0])
    # never adapted, not adapting: eps unchanged
    _, _, st4 = run_decide(lib, dtype, C, k, l0, l1, u, state_block(), adapting=0)
    assert float(st4[0]) == EPS and float(st4[2]) == 0.0

    # non-finite log joints (and, through them, energies) at chosen chains: those reject with a = 0, the others keep their bits
    bad = [(0, float("nan"))] if C == 1 else [(0, float("nan")), (C // 2, float("inf")), (C - 1, float("-inf"))]
    l1b = l1.clone()
    for c, v in bad:
        l1b[c] = v
    outb, accb, stb = run_decide(lib, dtype, C, k, l0, l1b, u, state_block(), adapting=1)
    idx = torch.tensor([c for c, _ in bad])
    assert bool((accb[idx] == 0).all()) and bool((outb[0][idx] == 0.0).all())
    assert torch.equal(outb[4][idx], l0.double()[idx])
    keep = torch.ones(C, dtype=torch.bool)
    keep[idx] = False
    assert torch.equal(accb[keep], acc[keep])
    for r in range(5):
        assert torch.equal(outb[r][keep], out[r][keep])
    assert bool(torch.isfinite(stb).all())
    close40(stb[6:7], (t["a"][keep].sum() / C).view(1))
    # a non-finite kinetic partial does the same
    kb = [x.clone() for x in k]
    kb[3][0, 1] = float("inf")
    outk, acck, stk = run_decide(lib, dtype, C, kb, l0, l1, u, state_block(), adapting=1)
    assert int(acck[0]) == 0 and float(outk[0][0]) == 0.0 and bool(torch.isfinite(stk).all())
    assert torch.equal(acck[1:], acc[1:]) and torch.equal(outk[:, 1:], out[:, 1:])


@pytest.mark.parametrize("C", [1, 3, 65, 257])
def test_drawn_uniforms_are_the_main_librarys_philox_stream(lib, C):
    k, l0, l1, _ = decide_inputs(C, 5)
    seed, call = 0xABCDEF12345, 17
    rs = torch.tensor([99, 1 << 20], dtype=torch.int64, device=DEV)
    for kw, stream_args in [(dict(seed=seed, call=call), (seed, call, None)), (dict(seed=1, call=3, rs=rs), (1, 3, rs))]:
        drawn = run_decide(lib, F32, C, k, l0, l1, None, state_block(), adapting=1, **kw)
        u = philox("zs_philox_uniform_f32", C, *stream_args)
        given = run_decide(lib, F32, C, k, l0, l1, u, state_block(), adapting=1)
        assert all(torch.equal(a, b) for a, b in zip(drawn, given))


# ------------------------------------------------------------------------------------------------ 4. select
@pytest.mark.parametrize("dtype", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("C,rows", [(1, [5]), (3, [5, 7]), (65, [64]), (257, [1]), (3, [4] * 32), (2, [1023, 1025, 2, 2047])],
                         ids=["one", "5+7", "vector", "row1", "32x4", "tile_edges"])
def test_select_is_exactly_where(lib, C, rows, dtype):
    sizes = [C * r for r in rows]
    starts = [int(x) for x in np.cumsum([0] + sizes)]
    n = starts[-1]
    q0, q, _, _ = inputs(n, dtype, 13)
    gen = torch.Generator().manual_seed(C)
    accept = (torch.rand(C, generator=gen) < 0.5).to(torch.int32)
    want = torch.cat([torch.where(accept.bool().view(C, 1), q[s:s + k].view(C, -1), q0[s:s + k].view(C, -1)).reshape(-1)
                      for s, k in zip(starts, sizes)])
    for shift in (0, 1):
        ar = Arena(shift)
        v0, v1, vo = place(ar, q0, sizes), place(ar, q, sizes), place(ar, torch.zeros_like(q), sizes)
        table = [dict(q0=v0[i], q=v1[i], q_out=vo[i], start=starts[i], row=rows[i]) for i in range(len(rows))]
        assert raw_select(lib, dtype, table, n, C, accept.to(DEV)) == 0
        ar.check_guards()
        assert torch.equal(cat(vo), want) and torch.equal(cat(v0), q0) and torch.equal(cat(v1), q)
        # in place: q_out = q0
        table = [dict(q0=v0[i], q=v1[i], q_out=v0[i], start=starts[i], row=rows[i]) for i in range(len(rows))]
        assert raw_select(lib, dtype, table, n, C, accept.to(DEV)) == 0
        torch.cuda.synchronize()
        assert torch.equal(cat(v0), want)


# ------------------------------------------------------------------------------------------------ 5. edges
def test_rejected_arguments_and_empty_launches_write_nothing(lib):
    t = dict((k, torch.full((8,), SENTINEL, device=DEV)) for k in ("q0", "q", "p", "grad", "p0", "q_out", "ksum"))
    st = state_block()
    acc = torch.full((4,), 777, dtype=torch.int32, device=DEV)
    out = torch.full((20,), SENTINEL, dtype=F64, device=DEV)
    lp = torch.full((4,), SENTINEL, device=DEV)
    row = dict(q0=t["q0"], q=t["q"], p=t["p"], grad=t["grad"], z=None, p0=t["p0"], q_out=t["q_out"], start=0, row=2)

    def mv(kind, rows, n, C, state=st, ksum=t["ksum"], **kw):
        return raw_move(lib, F32, kind, rows, n, C, state, ksum, **kw)
    # empty
    assert mv(BEGIN, [], 0, 4) == 0 and mv(BEGIN, [row], 0, 4) == 0 and mv(END, [row], 8, 0) == 0
    assert raw_select(lib, F32, [row], 0, 4, acc) == 0 and raw_select(lib, F32, [row], 8, 0, acc) == 0
    assert raw_decide(lib, F32, [(t["ksum"], t["ksum"], 1, 0)], 0, lp, lp, None, st, out, acc) == 0
    # rejected
    many = [dict(row, start=i, row=1) for i in range(33)]
    assert mv(BEGIN, many, 33, 1) == ENOTSUP
    assert raw_select(lib, F32, many, 33, 1, acc) == ENOTSUP
    assert raw_decide(lib, F32, [(t["ksum"], t["ksum"], 1, 0)] * 17, 4, lp, lp, None, st, out, acc) == ENOTSUP
    assert mv(3, [row], 8, 4) == EINVAL and mv(-1, [row], 8, 4) == EINVAL                     # unknown kind
    assert mv(BEGIN, [row], 8, 4, state=None) == EINVAL
    assert mv(BEGIN, [row], 8, 4, ksum=None) == EINVAL and mv(END, [row], 8, 4, ksum=None) == EINVAL
    for kind, missing in [(BEGIN, "q0"), (BEGIN, "q"), (BEGIN, "p"), (BEGIN, "grad"), (STEP, "q"), (STEP, "p"), (STEP, "grad"),
                          (END, "p"), (END, "grad")]:
        assert mv(kind, [dict(row, **{missing: None})], 8, 4) == EINVAL, (kind, missing)
    assert mv(BEGIN, [dict(row, row=3)], 8, 4) == EINVAL                                     # row not dividing the tensor
    assert mv(BEGIN, [dict(row, row=0)], 8, 4) == EINVAL
    assert mv(BEGIN, [row], 8, 3) == EINVAL                                                   # 8 elements are not 3 chains of 2
    assert mv(BEGIN, [row, dict(row, start=0)], 8, 4) == EINVAL                               # starts not ascending
    assert mv(BEGIN, [dict(row, start=1)], 8, 4) == EINVAL                                    # not 0-based
    assert mv(BEGIN, [row], -1, 4) == EINVAL and mv(BEGIN, [row], 8, -1) == EINVAL
    for missing in ("q0", "q", "q_out"):
        assert raw_select(lib, F32, [dict(row, **{missing: None})], 8, 4, acc) == EINVAL
    assert raw_select(lib, F32, [row], 8, 4, None) == EINVAL
    assert raw_select(lib, F32, [dict(row, row=3)], 8, 4, acc) == EINVAL
    ch = (t["ksum"], t["ksum"], 1, 0)
    assert raw_decide(lib, F32, [], 4, lp, lp, None, st, out, acc) == EINVAL
    assert raw_decide(lib, F32, [(None, t["ksum"], 1, 0)], 4, lp, lp, None, st, out, acc) == EINVAL
    assert raw_decide(lib, F32, [(t["ksum"], t["ksum"], 0, 0)], 4, lp, lp, None, st, out, acc) == EINVAL
    assert raw_decide(lib, F32, [ch], 4, None, lp, None, st, out, acc) == EINVAL
    assert raw_decide(lib, F32, [ch], 4, lp, None, None, st, out, acc) == EINVAL
    assert raw_decide(lib, F32, [ch], 4, lp, lp, None, None, out, acc) == EINVAL
    assert raw_decide(lib, F32, [ch], 4, lp, lp, None, st, None, acc) == EINVAL
    assert raw_decide(lib, F32, [ch], 4, lp, lp, None, st, out, None) == EINVAL
    assert raw_decide(lib, F32, [ch], 4, lp, lp, None, st, out, acc, adapting=1, delta=1.5) == EINVAL
    assert raw_decide(lib, F32, [ch], 4, lp, lp, None, st, out, acc, adapting=1, gamma=0.0) == EINVAL
    assert raw_decide(lib, F32, [ch], 4, lp, lp, None, st, out, acc, adapting=1, kappa=0.25) == EINVAL
    torch.cuda.synchronize()
    assert all(bool((x == SENTINEL).all()) for x in t.values()) and bool((out == SENTINEL).all()) and bool((acc == 777).all())
    assert torch.equal(st.cpu(), state_block().cpu()), "a rejected or empty call wrote something"

    def ksum_slots(rows):          # the C entry's own count (the binding's ksum_slots() is its Python restatement)
        return lib.raw("zs_hmc_ksum_slots", (ctypes.c_int64 * len(rows))(*rows), len(rows))
    assert ksum_slots([1, 1024, 1025, 1026]) == 1 + 2 + 2 + 3 and ksum_slots([5, 0]) == -1
