"""The fused sampler update through the raw C ABI of libzs_mcmc.so (include/zs_mcmc.h), on the GPU.

Truth: a float64 torch evaluation of the header's formulas on the same inputs.  Bound: |err| <= 2^-20 S for _f32, S being
the sum of the absolute values of the terms added for that element (for q' of SGHMC_POST: q and the terms of v').  That
allows sixteen float32 roundings of 2^-24 relative each; the formulas have at most nine operations and the hardware sqrt,
rcp and exp2 are 1 ulp.  _f64 is held to 2^-48 S in the same way (thirty-two roundings of 2^-53, shared between the
kernel and the float64 truth itself).  Inputs are fixed-seed and of order 1; PSGLD's second moment is >= 0 with exact zeros."""
import ctypes

import numpy as np
import pytest
import torch

from kernel_abi import DEV, EINVAL, ENOTSUP, SENTINEL, Arena, load, ptr, stream

pytestmark = pytest.mark.gpu

HYPER = dict(lr=1e-2, decay=0.9, epsilon=1e-3, alpha=0.3, beta=0.02)
SGLD, PSGLD, PRE, POST = 0, 1, 2, 3
SECOND, RESAMPLE = 1, 2
# (kind, flags) of every form of the update
FORMS = [(SGLD, 0), (PSGLD, 0), (PRE, RESAMPLE), (PRE, SECOND), (PRE, SECOND | RESAMPLE), (POST, 0), (POST, SECOND)]


@pytest.fixture(scope="module")
def lib():
    return load("mcmc")


def raw(lib, dtype, kind, rows, n, flags=0, seed=0, call=0, rs=None, hyper=None, n_tensors=None):
    """rows: (q_in, q_out, grad, state, z, start) per tensor (tensors, None, or raw addresses); returns the entry point's code."""
    from zhusuan import _mcmc_hip
    h = dict(HYPER, **(hyper or {}))
    table = (_mcmc_hip.McmcTensor * max(len(rows), 1))()
    for e, r in zip(table, rows):
        e.q_in, e.q_out, e.grad, e.state, e.z = [ptr(t) for t in r[:5]]
        e.start = r[5]
    name = "zs_mcmc_update_f32" if dtype == torch.float32 else "zs_mcmc_update_f64"
    return lib.raw(name, kind, table if rows else None, len(rows) if n_tensors is None else n_tensors, n, h["lr"], h["decay"],
                   h["epsilon"], h["alpha"], h["beta"], flags, seed, call, ptr(rs), stream())


def truth(kind, flags, q, g, s, z, h=HYPER):
    """float64: (q', s', S_q, S_s)."""
    q, g, s, z = [t.double() for t in (q, g, s, z)]
    lr, second, resample = h["lr"], bool(flags & SECOND), bool(flags & RESAMPLE)
    if kind == SGLD:
        terms = [q, 0.5 * lr * g, np.sqrt(lr) * z]
        return sum(terms), s, sum(t.abs() for t in terms), s.abs()
    if kind == PSGLD:
        ta = [h["decay"] * s, (1.0 - h["decay"]) * g * g]
        a = ta[0] + ta[1]
        G = 1.0 / (h["epsilon"] + torch.sqrt(a))
        terms = [q, 0.5 * lr * G * g, torch.sqrt(lr * G) * z]
        return sum(terms), a, sum(t.abs() for t in terms), ta[0].abs() + ta[1].abs()
    if kind == PRE:
        v = np.sqrt(lr) * z if resample else s
        terms = [q, 0.5 * v] if second else [q]
        return sum(terms), v, sum(t.abs() for t in terms), v.abs()
    noise = np.sqrt(2.0 * (h["alpha"] - h["beta"]) * lr)
    if second:
        d = np.exp(-0.5 * h["alpha"])
        tv = [d * d * s, d * lr * g, d * noise * z]
        v = sum(tv)
        Sv = sum(t.abs() for t in tv)
        return q + 0.5 * v, v, q.abs() + 0.5 * Sv, Sv
    tv = [(1.0 - h["alpha"]) * s, lr * g, noise * z]
    v = sum(tv)
    Sv = sum(t.abs() for t in tv)
    return q + v, v, q.abs() + Sv, Sv


def within(got, want, S, dtype):
    rel = 2.0 ** -20 if dtype == torch.float32 else 2.0 ** -48
    err = (got.double() - want).abs()
    bad = err > rel * S
    assert not bool(bad.any()), (float(err.max()), float((err / S.clamp_min(1e-300)).max()), rel)


def inputs(n, dtype, seed):
    """q, g, state (kind-appropriate: >= 0 with exact zeros for PSGLD is made by the caller), z -- flat, on the host."""
    gen = torch.Generator().manual_seed(seed)
    q, g, s, z = [torch.randn(n, generator=gen, dtype=torch.float64).to(dtype) for _ in range(4)]
    return q, g, s, z


def state_for(kind, s):
    if kind != PSGLD:
        return s
    a = s.abs()
    a[::3] = 0.0
    return a


def run_layout(lib, dtype, kind, flags, sizes, offsets, data, inject, seed=5, call=9, rs=None):
    """The update on tensors laid out as (sizes, offsets): every piece of every operand inside a guarded buffer of its own,
    offsets[i] extra leading elements shifting the pieces of tensor i off their alignment; returns flat (q', s') on the host."""
    q, g, s, z = data
    starts = [int(x) for x in np.cumsum([0] + list(sizes))]
    arenas = [Arena(shift) for shift in (offsets or [0] * len(sizes))]          # one per tensor: the shift is the arena's

    def place(flat):
        return [ar.put(piece) for ar, piece in zip(arenas, torch.split(flat, sizes))]
    qi, qo, gg, ss, zz = [place(t) for t in (q, torch.zeros_like(q), g, s, z)]
    rows = [(qi[i], qo[i], gg[i], ss[i], zz[i] if inject else None, starts[i]) for i in range(len(sizes))]
    rc = raw(lib, dtype, kind, rows, starts[-1], flags=flags, seed=seed, call=call, rs=rs)
    assert rc == 0, rc
    for ar in arenas:
        ar.check_guards()
    for a, b in zip(qi, place(q)):
        assert torch.equal(a, b), "q_in was modified"
    return torch.cat([t.cpu() for t in qo]), torch.cat([t.cpu() for t in ss])


def philox(n, seed, call, rs=None):
    """Elements [0, n) of the MAIN library's zs_philox_normal_f32 stream."""
    from zhusuan import _hip
    out = torch.empty(n, dtype=torch.float32, device=DEV)
    _hip.lib().call("zs_philox_normal_f32", out.data_ptr(), n, seed, call, ptr(rs), _hip.stream_for(out))
    torch.cuda.synchronize()
    return out.cpu()


# ------------------------------------------------------------------------------------------------ 1. truth
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind,flags", FORMS)
def test_every_kind_matches_the_float64_formulas(lib, kind, flags, dtype):
    n = 4096 + 8
    q, g, s, z = inputs(n, dtype, 100 + 10 * kind + flags)
    s = state_for(kind, s)
    for sizes, offsets in [([n], None), ([1001, n - 1001], [1, 0])]:          # vector form, element form
        q2, s2 = run_layout(lib, dtype, kind, flags, sizes, offsets, (q, g, s, z), inject=True)
        wq, ws, Sq, Ss = truth(kind, flags, q, g, s, z)
        within(q2, wq, Sq, dtype)
        if kind != SGLD:
            within(s2, ws, Ss, dtype)
        else:
            assert torch.equal(s2, s)
    if kind == PRE and flags == RESAMPLE:
        # first order: q unchanged, v = sqrt(lr) z exactly (one multiply by the rounded scalar)
        assert torch.equal(q2, q)
        c = torch.tensor(np.sqrt(HYPER["lr"]), dtype=torch.float64).to(dtype)
        assert torch.equal(s2, c * z)


# ------------------------------------------------------------------------------------------------ 2. stream
@pytest.mark.parametrize("sizes", [[5, 7], [8, 12]], ids=["element", "vector"])
@pytest.mark.parametrize("kind,flags", [(SGLD, 0), (PSGLD, 0), (PRE, RESAMPLE), (POST, SECOND)])
def test_kernel_noise_is_the_main_librarys_philox_stream(lib, kind, flags, sizes):
    n = sum(sizes)
    q, g, s, _ = inputs(n, torch.float32, 7)
    s = state_for(kind, s)
    zero = torch.zeros(n)
    seed, call = 0x1234ABCD5678, 41
    rs = torch.tensor([99, 1 << 20], dtype=torch.int64, device=DEV)          # {seed, non-zero base}
    for kw, stream_args in [(dict(seed=seed, call=call), (seed, call, None)),
                            (dict(seed=1, call=3, rs=rs), (1, 3, rs)),
                            (dict(seed=seed, call=call + 1), (seed, call + 1, None))]:
        drawn = run_layout(lib, torch.float32, kind, flags, sizes, None, (q, g, s, zero), inject=False, **kw)
        z = philox(n, *stream_args)
        given = run_layout(lib, torch.float32, kind, flags, sizes, None, (q, g, s, z), inject=True, seed=0, call=0)
        assert torch.equal(drawn[0], given[0]) and torch.equal(drawn[1], given[1])
        if kw.get("call") == call:
            first = drawn
    assert not torch.equal(first[0] if kind != PRE else first[1], drawn[0] if kind != PRE else drawn[1]), "call + 1 drew the same noise"


# ------------------------------------------------------------------------------------------------ 3. shapes
LAYOUTS = [("n1", [1], None), ("n3", [3], None), ("n4", [4], None), ("n5", [5], None), ("5+7", [5, 7], None),
           ("8+12", [8, 12], None), ("offset_view", [16], [1]), ("32x4", [4] * 32, None),
           ("grid_stride_and_tail", [1048576 + 5], None)]


@pytest.mark.parametrize("name,sizes,offsets", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_layouts_agree_bit_for_bit_with_the_vector_form(lib, name, sizes, offsets):
    """Every layout against ONE aligned tensor holding the same flat data padded to a multiple of four (the vector form), noise
    from the Philox stream: the same flat element draws the same normal and rounds alike on either path."""
    n = sum(sizes)
    npad = (n + 3) // 4 * 4
    forms = FORMS if n < 1000 else [(PSGLD, 0), (POST, SECOND)]
    z = philox(npad, 5, 9)
    for kind, flags in forms:
        q, g, s, _ = inputs(npad, torch.float32, 31 + kind)
        s = state_for(kind, s)
        a = run_layout(lib, torch.float32, kind, flags, sizes, offsets, (q[:n], g[:n], s[:n], z[:n]), inject=False)
        b = run_layout(lib, torch.float32, kind, flags, [npad], None, (q, g, s, z), inject=False)
        assert torch.equal(a[0], b[0][:n]) and torch.equal(a[1], b[1][:n]), (name, kind, flags)
        wq, ws, Sq, Ss = truth(kind, flags, q[:n], g[:n], s[:n], z[:n])
        within(a[0], wq, Sq, torch.float32)
        if kind != SGLD and not (kind == PRE and not flags & RESAMPLE):
            within(a[1], ws, Ss, torch.float32)


# ------------------------------------------------------------------------------------------------ 4. edges
def test_rejected_arguments_and_empty_launch(lib):
    f32 = torch.float32
    t = [torch.full((8,), SENTINEL, device=DEV) for _ in range(4)]
    row = (t[0], t[1], t[2], t[3], None, 0)
    assert raw(lib, f32, SGLD, [], 0) == 0
    assert raw(lib, f32, PSGLD, [row], 0) == 0
    torch.cuda.synchronize()
    assert all(bool((x == SENTINEL).all()) for x in t), "n = 0 wrote something"
    many = [(t[0], t[1], t[2], t[3], None, i) for i in range(33)]
    assert raw(lib, f32, SGLD, many, 33) == ENOTSUP
    assert raw(lib, f32, SGLD, [row], 8, hyper=dict(lr=-1e-3)) == EINVAL
    assert raw(lib, f32, SGLD, [(None,) + row[1:]], 8) == EINVAL
    assert raw(lib, f32, PSGLD, [row], 8, hyper=dict(decay=1.0)) == EINVAL
    assert raw(lib, f32, PSGLD, [row], 8, hyper=dict(decay=-0.1)) == EINVAL
    assert raw(lib, f32, POST, [row], 8, hyper=dict(alpha=0.01, beta=0.02)) == EINVAL
    assert raw(lib, f32, 7, [row], 8) == EINVAL
    assert raw(lib, f32, PSGLD, [(t[0], t[1], t[2], None, None, 0)], 8) == EINVAL          # PSGLD without its state
    assert raw(lib, f32, SGLD, [(t[0], t[1], None, None, None, 0)], 8) == EINVAL            # SGLD without a gradient
    assert raw(lib, f32, SGLD, [row, (t[0], t[1], t[2], t[3], None, 0)], 8) == EINVAL       # starts not ascending
    torch.cuda.synchronize()
    assert all(bool((x == SENTINEL).all()) for x in t), "a rejected call wrote something"


@pytest.mark.parametrize("kind,flags", [(SGLD, 0), (PSGLD, 0), (POST, SECOND), (PRE, SECOND | RESAMPLE)])
def test_in_place_equals_out_of_place(lib, kind, flags):
    n = 24
    q, g, s, z = inputs(n, torch.float32, 77)
    s = state_for(kind, s)
    out = run_layout(lib, torch.float32, kind, flags, [n], None, (q, g, s, z), inject=True)
    d = [x.to(DEV) for x in (q, g, s, z)]
    assert raw(lib, torch.float32, kind, [(d[0], d[0], d[1], d[2], d[3], 0)], n, flags=flags) == 0
    torch.cuda.synchronize()
    assert torch.equal(d[0].cpu(), out[0]) and torch.equal(d[2].cpu(), out[1])
