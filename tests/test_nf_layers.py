"""``zhusuan.transform.PlanarFlow`` / ``HouseholderFlow`` on both back-ends (``ndev``: the torch restatements of tests/nf_host.py on
the host, the kernels of include/zs_nf.h on the GPU).  See tests/README_nf.md.

Truth for values and gradients: the op sequence of the example's own ``PF`` / ``HF`` modules (examples/flow_vae.py) in float64 --
for more than one planar layer those ``PF`` layers applied in a loop with the log-dets summed -- held within 16 x that sequence's
own float32-vs-float64 distance (the suite's rule for gradients).  The float32 run of the sequence is made on the device under
test: the modules' linear layers and the reductions of their backward are torch's on that device, so its float32 behaviour is
part of what the distance has to measure (on the MI355X the CPU's float32 run of the Householder chain at B = 5, D = 2, L = 3
happens to land within half an ulp of the truth, 21.6 times closer than the module, whose kernels hold their derived bounds in
tests/test_nf_kernel.py); the float64 truth is computed on the CPU."""
import inspect

import pytest
import torch

import host_backend
import nf_host
from nf_host import ndev  # noqa: F401
from truth import gen, held_to_the_rule

F32, F64 = torch.float32, torch.float64
WORST = {}


# ------------------------------------------------------------------------------------------------ the example's op sequence
def example_planar(z, u, w, b):
    """examples.flow_vae.PF.forward, layer after layer, the log-dets summed.  u, w [L, D], b [L]."""
    import torch.nn.functional as F
    total = 0.0
    for l in range(u.shape[0]):
        ul, wl, bl = u[l:l + 1], w[l:l + 1], b[l:l + 1]
        wu = (wl * ul).sum()
        w_unit_sq = wl / (wl * wl).sum()
        u_hat = ul + (F.softplus(wu) - 1. - wu) * w_unit_sq
        t = torch.tanh(z @ wl.t() + bl)
        slope = (1. - t * t) * (wl * u_hat).sum()
        z, total = z + u_hat * t, total + torch.log(torch.abs(1. + slope))
    return z, total


def example_householder(z, aux, weights, biases):
    """examples.flow_vae.HF._forward, layer after layer."""
    v = aux
    for W, c in zip(weights, biases):
        v = torch.nn.functional.linear(v, W, c)
        along = (v * z).sum(1, keepdim=True) / (v * v).sum(1, keepdim=True)
        z = z - 2. * along * v
    return z


def grads_of(outs, cots, leaves):
    loss = sum((o * c).sum() for o, c in zip(outs, cots))
    return torch.autograd.grad(loss, leaves)


def check(name, got, t32, t64):
    held_to_the_rule(name[0], zip(name[1], got, t32, t64), WORST)


# ------------------------------------------------------------------------------------------------ surface
def test_import_forms_signatures_and_state_dict():
    import zhusuan as zs
    import zhusuan.transform as T
    assert zs.transform is T and zs.PlanarFlow is T.PlanarFlow and zs.HouseholderFlow is T.HouseholderFlow
    assert sorted(T.__all__) == ["HouseholderFlow", "PlanarFlow"]
    sp = inspect.signature(T.PlanarFlow.__init__).parameters
    assert list(sp) == ["self", "z_dim", "n_flows", "name"] and sp["n_flows"].default == 1 and sp["name"].default is None
    sh = inspect.signature(T.HouseholderFlow.__init__).parameters
    assert list(sh) == ["self", "z_dim", "v_dim", "n_flows", "name"] and sh["name"].default is None
    pf = T.PlanarFlow(7, 3)
    assert {k: tuple(v.shape) for k, v in pf.state_dict().items()} == {"u": (3, 7), "w": (3, 7), "b": (3,)}
    hf = T.HouseholderFlow(7, 4, 3)
    assert {k: tuple(v.shape) for k, v in hf.state_dict().items()} == {
        "v_layers.0.weight": (7, 4), "v_layers.0.bias": (7,), "v_layers.1.weight": (7, 7), "v_layers.1.bias": (7,),
        "v_layers.2.weight": (7, 7), "v_layers.2.bias": (7,)}
    assert isinstance(hf.v_layers, torch.nn.ModuleList)
    for bad in ((0, 1), (3, 0), (-1, 2)):
        with pytest.raises(ValueError):
            T.PlanarFlow(*bad)
        with pytest.raises(ValueError):
            T.HouseholderFlow(bad[0], 4, bad[1])
    assert "not been evaluated" in zs.explain(pf)


def test_import_zhusuan_does_not_need_the_library():
    import subprocess
    import sys
    from conftest import PKG_ROOT
    code = ("import sys; sys.path.insert(0, %r); import zhusuan, zhusuan.transform; from zhusuan import _nf_hip; "
            "assert _nf_hip._LIB is None; _nf_hip.LIB_PATH = '/nonexistent/libzs_nf.so'; zhusuan.PlanarFlow(3, 2); "
            "zhusuan.HouseholderFlow(3, 2, 2); assert _nf_hip._LIB is None; print('ok')" % PKG_ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
    from zhusuan import _nf_hip
    with pytest.raises(RuntimeError, match="make -C zhusuan-pytorch_amd/csrc nf"):
        _nf_hip.lib("/nonexistent/libzs_nf.so")
    assert _nf_hip.ABI_VERSION == 1 and _nf_hip.MAX_DIM == 64 and _nf_hip.MAX_LAYERS == 32


def test_a_single_planar_layer_has_the_parameter_bits_of_the_example():
    import zhusuan as zs
    from examples import flow_vae
    torch.manual_seed(0)
    mine = zs.PlanarFlow(5, 1)
    torch.manual_seed(0)
    theirs = flow_vae.PlanarFlow(5, 1).flows[0]
    assert torch.equal(mine.u, theirs.u) and torch.equal(mine.w, theirs.w) and torch.equal(mine.b, theirs.b)
    torch.manual_seed(0)
    deep = zs.PlanarFlow(5, 3)          # layer by layer, u_l, w_l, b_l
    assert torch.equal(deep.u[0], mine.u[0]) and torch.equal(deep.w[0], mine.w[0]) and torch.equal(deep.b[:1], mine.b)


@pytest.mark.gpu
def test_a_host_tensor_raises():
    import zhusuan as zs
    nf_host.uninstall()
    host_backend.uninstall()
    with pytest.raises(RuntimeError, match="no CPU path"):
        zs.PlanarFlow(3, 2)(torch.zeros(4, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):
        zs.HouseholderFlow(3, 2, 2)((torch.zeros(4, 3), torch.zeros(4, 2)))


# ------------------------------------------------------------------------------------------------ values and gradients
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("D", [2, 7, 40])
@pytest.mark.parametrize("B", [1, 5])
def test_planar_values_and_gradients(ndev, B, D, L, dtype):
    import zhusuan as zs
    torch.manual_seed(100 * D + 10 * B + L)
    flow = zs.PlanarFlow(D, L)
    with torch.no_grad():
        flow.w.sub_(0.5)
        flow.u.sub_(0.5)
    g = gen(7 * D + B)
    z0, gy, gld = torch.randn(B, D, generator=g), torch.randn(B, D, generator=g), torch.randn(B, 1, generator=g)

    def sequence(dt, where):
        leaves = [t.detach().to(where).to(dt).requires_grad_() for t in (z0, flow.u, flow.w, flow.b)]
        y, ld = example_planar(*leaves)
        out = [y.detach(), ld.detach()] + list(grads_of((y, ld), (gy.to(where).to(dt), gld.to(where).to(dt)), leaves))
        return [t.cpu() for t in out]
    t32, t64 = sequence(F32, ndev), sequence(F64, "cpu")
    flow = flow.to(ndev).to(dtype)
    z = z0.to(ndev).to(dtype).requires_grad_()
    y, ld = flow(z)
    assert y.shape == (B, D) and ld.shape == (B, 1) and y.dtype == dtype and ld.dtype == dtype
    assert "P1 zs_nf_planar_fwd" in zs.explain(flow) and flow.last_path["why"] is None
    got = [y, ld] + list(grads_of((y, ld), (gy.to(ndev).to(dtype), gld.to(ndev).to(dtype)), [z, flow.u, flow.w, flow.b]))
    if dtype == F64:          # the float64 kernels against the float64 sequence: its float32 distance is a generous bar, 1e-12 the real one
        for a, c in zip(got, t64):
            assert float((a.detach().cpu() - c).abs().max()) <= 1e-12 * (1.0 + float(c.abs().max()))
    check(("planar", ("z_out", "log_det", "dz", "du", "dw", "db")), got, t32, t64)


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("D", [2, 7, 40])
@pytest.mark.parametrize("B", [1, 5])
def test_householder_values_and_gradients(ndev, B, D, L, dtype):
    import zhusuan as zs
    V = 4
    torch.manual_seed(100 * D + 10 * B + L)
    flow = zs.HouseholderFlow(D, V, L)
    g = gen(9 * D + B)
    z0, aux0, gy = torch.randn(B, D, generator=g), torch.randn(B, V, generator=g), torch.randn(B, D, generator=g)
    params = [p for layer in flow.v_layers for p in (layer.weight, layer.bias)]

    def sequence(dt, where):
        leaves = [t.detach().to(where).to(dt).requires_grad_() for t in [z0, aux0] + params]
        y = example_householder(leaves[0], leaves[1], leaves[2::2], leaves[3::2])
        return [t.cpu() for t in [y.detach()] + list(grads_of((y,), (gy.to(where).to(dt),), leaves))]
    t32, t64 = sequence(F32, ndev), sequence(F64, "cpu")
    flow = flow.to(ndev).to(dtype)
    z, aux = z0.to(ndev).to(dtype).requires_grad_(), aux0.to(ndev).to(dtype).requires_grad_()
    y, ld = flow((z, aux))
    assert y.shape == (B, D) and ld.shape == (1, 1) and float(ld) == 0.0 and ld.device == y.device
    assert "H1 zs_nf_householder_fwd" in zs.explain(flow)
    dev_params = [p for layer in flow.v_layers for p in (layer.weight, layer.bias)]
    got = [y] + list(grads_of((y,), (gy.to(ndev).to(dtype),), [z, aux] + dev_params))
    names = ("z_out", "dz", "daux") + tuple("dv_layers.%d.%s" % (l, n) for l in range(L) for n in ("weight", "bias"))
    check(("householder", names), got, t32, t64)


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("D", [1, 3, 17])
def test_gradcheck_of_the_f64_functions(D, L):
    from zhusuan.transform import _functions as F_
    nf_host.uninstall()
    host_backend.uninstall()
    dev, g = torch.device("cuda:0"), gen(D + 10 * L)
    mk = lambda *s: (0.7 * torch.randn(*s, generator=g, dtype=F64)).to(dev).requires_grad_()  # noqa: E731
    assert torch.autograd.gradcheck(F_.PlanarStack.apply, (mk(4, D), mk(L, D), mk(L, D) + 1.0, mk(L)), eps=1e-6, atol=1e-7, rtol=1e-5,
                                    nondet_tol=0.0)
    assert torch.autograd.gradcheck(F_.HouseholderStack.apply, (mk(4, D), mk(L, 4, D)), eps=1e-6, atol=1e-7, rtol=1e-5, nondet_tol=0.0)


# ------------------------------------------------------------------------------------------------ launches
def names_of(calls):
    return [c[0] for c in calls]


def test_planar_launch_budget_and_null_operands(ndev):
    import zhusuan as zs
    torch.manual_seed(1)
    flow = zs.PlanarFlow(7, 3).to(ndev)
    z = torch.randn(5, 7, generator=gen(2)).to(ndev)
    with nf_host.recording() as calls:
        y, ld = flow(z.clone().requires_grad_())
        assert names_of(calls) == ["planar_fwd"]
        del calls[:]
        (y.sum() + ld.sum()).backward()
        assert names_of(calls) == ["planar_bwd", "planar_finish"]
        assert calls[0][2]["gy"] == (5, 7) and calls[0][2]["gld"] == (5,) and calls[0][2]["want_gx"] and calls[0][2]["want_partials"]
        # an output that did not enter the loss passes NULL, not zeros
        for use, gy, gld in ((lambda y, ld: y.sum(), (5, 7), None), (lambda y, ld: ld.sum(), None, (5,))):
            del calls[:]
            use(*flow(z.clone().requires_grad_())).backward()
            assert names_of(calls) == ["planar_fwd", "planar_bwd", "planar_finish"]
            assert calls[1][2]["gy"] == gy and calls[1][2]["gld"] == gld
        # only z requires grad: one launch, no partials
        for p in flow.parameters():
            p.requires_grad_(False)
        del calls[:]
        y, ld = flow(z.clone().requires_grad_())
        (y.sum() + ld.sum()).backward()
        assert names_of(calls) == ["planar_fwd", "planar_bwd"] and not calls[1][2]["want_partials"] and calls[1][2]["want_gx"]
        # only the parameters do: no gx
        for p in flow.parameters():
            p.requires_grad_(True)
        del calls[:]
        y, ld = flow(z)
        (y.sum() + ld.sum()).backward()
        assert names_of(calls) == ["planar_fwd", "planar_bwd", "planar_finish"] and not calls[1][2]["want_gx"]
        # a loss that reaches neither output launches nothing in backward
        del calls[:]
        zz = z.clone().requires_grad_()
        y, ld = flow(zz)
        (0.0 * zz.sum() + flow.b.sum()).backward()
        assert names_of(calls) == ["planar_fwd"]


def test_householder_launch_budget(ndev):
    import zhusuan as zs
    torch.manual_seed(1)
    flow = zs.HouseholderFlow(7, 4, 3).to(ndev)
    z, aux = torch.randn(5, 7, generator=gen(2)).to(ndev), torch.randn(5, 4, generator=gen(3)).to(ndev)
    with nf_host.recording() as calls:
        y, _ = flow((z.clone().requires_grad_(), aux))
        assert names_of(calls) == ["householder_fwd"] and calls[0][1][0] == (3, 5, 7)
        y.sum().backward()
        assert names_of(calls) == ["householder_fwd", "householder_bwd"] and calls[1][2] == {"want_gx": True, "want_gv": True}
        del calls[:]
        y, _ = flow((z, aux))
        y.sum().backward()
        assert names_of(calls) == ["householder_fwd", "householder_bwd"] and calls[1][2] == {"want_gx": False, "want_gv": True}
        del calls[:]
        y, _ = flow((z.clone().requires_grad_(), aux))
        flow.v_layers[0].bias.sum().backward()
        assert names_of(calls) == ["householder_fwd"]


def test_seventy_layers_run_as_three_chunks(ndev):
    import zhusuan as zs
    torch.manual_seed(3)
    flow = zs.PlanarFlow(5, 70)
    with torch.no_grad():
        flow.u.sub_(0.5).mul_(0.5)
        flow.w.sub_(0.5)
    z0 = torch.randn(4, 5, generator=gen(4))
    leaves = [t.detach().double().requires_grad_() for t in (z0, flow.u, flow.w, flow.b)]
    y64, ld64 = example_planar(*leaves)
    g64 = grads_of((y64, ld64), (torch.ones_like(y64), torch.ones_like(ld64)), leaves)
    flow = flow.to(ndev).double()
    z = z0.double().to(ndev).requires_grad_()
    with nf_host.recording() as calls:
        y, ld = flow(z)
        assert names_of(calls) == ["planar_fwd"] * 3 and [c[1][0][0] for c in calls] == [32, 32, 6]
        assert "70 layers in 3 launch(es)" in zs.explain(flow)
        del calls[:]
        got = grads_of((y, ld), (torch.ones_like(y), torch.ones_like(ld)), [z, flow.u, flow.w, flow.b])
        assert names_of(calls) == ["planar_bwd", "planar_finish"] * 3 and [c[1][0][0] for c in calls[::2]] == [6, 32, 32]
    for a, c in zip([y, ld] + list(got), [y64.detach(), ld64.detach()] + list(g64)):
        assert a.shape == c.shape
        assert float((a.detach().cpu() - c).abs().max()) <= 1e-11 * (1.0 + float(c.abs().max()))
    # Householder chunks the same way
    torch.manual_seed(5)
    hf = zs.HouseholderFlow(3, 2, 40).to(ndev).double()
    with nf_host.recording() as calls:
        out, _ = hf((z0[:, :3].double().to(ndev).requires_grad_(), torch.randn(4, 2, generator=gen(6)).double().to(ndev)))
        out.sum().backward()
    assert names_of(calls) == ["householder_fwd"] * 2 + ["householder_bwd"] * 2
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in hf.parameters())


def test_wide_rows_take_the_torch_composition(dev):
    """D = 65: no kernel call (the binding is not routed here: a call would raise on the host), and explain says why."""
    import zhusuan as zs
    torch.manual_seed(6)
    flow = zs.PlanarFlow(65, 2).to(dev)
    z = torch.randn(3, 65, generator=gen(7)).to(dev).requires_grad_()
    with nf_host.recording() as calls:
        y, ld = flow(z)
        (y.sum() + ld.sum()).backward()
        hf = zs.HouseholderFlow(65, 4, 2).to(dev)
        hy, hld = hf((z, torch.randn(3, 4, generator=gen(8)).to(dev)))
        hy.sum().backward()
    assert calls == []
    assert "torch composition" in zs.explain(flow) and "wider than 64" in zs.explain(flow) and flow.last_path["why"]
    assert "torch composition" in zs.explain(hf) and "wider than 64" in zs.explain(hf)
    y64, ld64 = example_planar(z.detach().cpu().double(), flow.u.detach().cpu().double(), flow.w.detach().cpu().double(),
                               flow.b.detach().cpu().double())
    assert float((y.detach().cpu() - y64).abs().max()) < 1e-4 and float((ld.detach().cpu() - ld64).abs().max()) < 1e-4
    assert ld.shape == (3, 1) and hld.shape == (1, 1) and flow.u.grad is not None and z.grad is not None


def test_the_name_form_and_the_tuple_input(ndev):
    import zhusuan as zs
    torch.manual_seed(8)
    z, aux = torch.randn(4, 5, generator=gen(9)).to(ndev), torch.randn(4, 3, generator=gen(10)).to(ndev)
    plain, named = zs.PlanarFlow(5, 2).to(ndev), zs.PlanarFlow(5, 2, name="z").to(ndev)
    named.load_state_dict(plain.state_dict())
    y, ld = plain(z)
    out, ld2 = named((z,))
    assert isinstance(out, dict) and list(out) == ["z"] and torch.equal(out["z"], y) and torch.equal(ld, ld2)
    y3, _ = plain((z, aux))          # a tuple: the first element is the latent
    assert torch.equal(y3, y)
    hp, hn = zs.HouseholderFlow(5, 3, 2).to(ndev), zs.HouseholderFlow(5, 3, 2, name="z").to(ndev)
    hn.load_state_dict(hp.state_dict())
    assert torch.equal(hn((z, aux))[0]["z"], hp((z, aux))[0])
    with pytest.raises(ValueError):
        plain(torch.zeros(4, 6, device=ndev))


@pytest.mark.gpu
def test_graphed_planar_vae_step_replays_equal_eager():
    """A small planar-VAE step captured by GraphedStep and replayed three times against eager training of a twin (rtol 2e-6 for
    the GEMMs' possible algorithm difference between eager and captured execution, as tests/test_flow_layers.py)."""
    import numpy as np
    import zhusuan as zs
    from zhusuan.variational.elbo import ELBO
    from examples import flow_vae, vae_mnist
    nf_host.uninstall()
    host_backend.uninstall()
    dev = torch.device("cuda:0")

    def make_model():
        torch.manual_seed(4)
        model = ELBO(vae_mnist.Generator(6, 5, 4, 8), flow_vae.Variational(6, 5, 4, 8), transform=zs.PlanarFlow(5, 3, name="z"),
                     transform_var=["z"]).to(dev)
        return model, zs.optim.FlatAdam(model.parameters(), lr=1e-3), zs.DeviceRNG(dev, seed=7)
    x = {"x": (torch.rand(4, 6, device=dev) < 0.5).float()}
    a, oa, ra = make_model()
    b, ob, rb = make_model()

    def compute_of(model, rng):
        def compute():
            rng.begin_step()
            for p in model.parameters():
                p.grad = None
            loss = model(x)
            loss.backward()
            return loss.detach()
        return compute
    step = zs.GraphedStep(compute_of(b, rb), ob.step, rng=rb, warmup=3, restore=True)
    assert step.captured
    eager = compute_of(a, ra)
    for _ in range(3):
        with zs.device_rng(ra):
            la = eager()
            oa.step()
        lb = step()
        torch.cuda.synchronize()
        np.testing.assert_allclose(float(lb), float(la), rtol=2e-6)
    for p, q in zip(a.parameters(), b.parameters()):
        np.testing.assert_allclose(q.detach().cpu().numpy(), p.detach().cpu().numpy(), rtol=2e-6, atol=1e-7)


@pytest.mark.gpu
def test_print_the_worst_multiples():
    for k in sorted(WORST):
        print("worst multiple of the sequence's own float32 distance  %-12s %-22s %.2f" % (k[0], k[1], WORST[k]))
