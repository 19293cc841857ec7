"""``zhusuan.invertible`` on both back-ends (``fdev``: the torch restatement of include/zs_flow.h on the host, the real kernels on
the GPU): the reference's interface, values and gradients of every layer, the in-place and log-det conventions and the
launch budget.

Truth: ``ref_forward`` below, the reference's op sequence (zhusuan/invertible/*.py of thuwzy/ZhuSuan-PyTorch) written out in
plain torch and run in float64 on a float64 copy of the layer's parameters.  Tolerance for float32: every value here is the
end of at most five layers of <= 3 GEMMs (inner dimension <= 8) and <= 7 element-wise operations each, order 1 in size:
fewer than 200 roundings of 2^-24, each amplified by at most the network's gain (< 8 for these fixed-seed weights), i.e.
< 1e-4 relative to the tensor's largest magnitude.  float64 inputs are held to 1e-12 in the same way."""
import copy

import pytest
import torch
import torch.nn as nn

import flow_host
import truth
from flow_host import fdev  # noqa: F401

TOL = {torch.float32: 1e-4, torch.float64: 1e-12}


def close(a, b, dtype, what=""):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    lim = TOL[dtype] * (1.0 + float(b.abs().max()) if b.numel() else 1.0)
    err = float((a - b).abs().max()) if b.numel() else 0.0
    assert err <= lim, (what, err, lim)


# ------------------------------------------------------------------------------------------------ the reference's ops
def ref_forward(layer, x, reverse=False):
    """(y, log_det) of ``layer`` by the reference's op sequence, in x's dtype, on a copy of x."""
    from zhusuan.invertible import MaskCoupling, Coupling, Scaling, RevSequential, MADE
    if isinstance(layer, RevSequential):
        items = []
        for f in (reversed(layer.layers) if reverse else layer.layers):
            x, ld = ref_forward(f, x, reverse)
            if ld is not None:
                items.append(ld)
        return x, sum(items) if items else torch.zeros([])
    if isinstance(layer, MaskCoupling):
        mask = layer.mask.to(x.dtype).to(x.device)
        kept, moved = mask * x, (1. - mask) * x
        delta = layer.nn(kept) * (1. - mask)
        return kept + (moved - delta if reverse else moved + delta), None
    if isinstance(layer, Coupling):
        # columns in pairs: position 0 of a pair is shifted when mask_config is set, position 1 otherwise; the other one feeds the net
        on_pos = 0 if layer.mask_config else 1
        cols = [x[:, 0::2], x[:, 1::2]]
        h = layer.in_block(cols[1 - on_pos])
        for blk in layer.mid_block:
            h = blk(h)
        shift = layer.out_block(h)
        cols[on_pos] = cols[on_pos] - shift if reverse else cols[on_pos] + shift
        return torch.stack(cols, dim=2).reshape(x.shape), None
    if isinstance(layer, Scaling):
        ld = torch.sum(layer.log_scale)
        return x * torch.exp(-layer.log_scale if reverse else layer.log_scale), ld
    if isinstance(layer, MADE):
        def net(v):
            h = nn.functional.linear(v, layer.net_input.weight * layer.net_input.mask, layer.net_input.bias)
            for m in layer.net:
                h = nn.functional.linear(h, m.weight * m.mask, m.bias) if hasattr(m, "mask") else m(h)
            return h
        if not reverse:
            m, loga = net(x).chunk(chunks=2, dim=1)
            return (x - m) * torch.exp(-loga), -loga
        out = torch.zeros_like(x)
        for i in layer.input_degrees:
            m, loga = net(out).chunk(chunks=2, dim=1)
            out = out.clone()
            out[:, i] = x[:, i] * torch.exp(loga[:, i]) + m[:, i]
        return out, loga
    raise TypeError(type(layer))


def make(kind, D, dev, dtype, seed=0):
    from zhusuan.invertible import MaskCoupling, Coupling, Scaling, RevSequential, MADE, get_coupling_mask
    torch.manual_seed(seed)
    if kind == "maskcoupling":
        layer = MaskCoupling(D, 8, 2, get_coupling_mask(D, 1, 1)[0])
    elif kind == "maskcoupling_nonbinary":
        layer = MaskCoupling(D, 8, 2, torch.tensor([0.25, -1.5, 1.0, 0.0, 0.5, 2.0, 1.0][:D]))
    elif kind == "coupling0":
        layer = Coupling(D, 8, 2, 0)
    elif kind == "coupling1":
        layer = Coupling(D, 8, 3, 1)
    elif kind == "scaling":
        layer = Scaling(D)
        with torch.no_grad():
            layer.log_scale.normal_()
    elif kind == "made":
        layer = MADE(D, 8, 2)
    elif kind == "made_tanh":
        layer = MADE(D, 8, 1, activation="tanh", input_order="random", input_degrees=torch.randperm(D))
    elif kind == "mixed":
        masks = get_coupling_mask(D, 1, 2, "Half")
        sc = Scaling(D)
        with torch.no_grad():
            sc.log_scale.normal_()
        layers = [MaskCoupling(D, 8, 2, masks[0]), MaskCoupling(D, 8, 1, masks[1]), sc]
        if D % 2 == 0:
            layers.insert(1, Coupling(D, 8, 2, 1))
        layer = RevSequential(layers)
    else:
        raise ValueError(kind)
    return layer.to(dev).to(dtype)


def double_twin(layer):
    twin = copy.deepcopy(layer).double().cpu()
    for m in twin.modules():
        if getattr(m, "mask", None) is not None and not isinstance(getattr(m, "mask"), nn.Parameter):
            m.mask = m.mask.double().cpu()
    return twin


KINDS = ["maskcoupling", "maskcoupling_nonbinary", "scaling", "made", "made_tanh", "mixed"]
CASES = [(k, B, D) for k in KINDS for B in (1, 5) for D in (2, 7)] + \
        [(k, B, D) for k in ("coupling0", "coupling1") for B in (1, 5) for D in (2, 6)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("kind,B,D", CASES, ids=["%s-B%d-D%d" % c for c in CASES])
def test_values_gradients_and_round_trip(fdev, kind, B, D, dtype):
    from zhusuan.invertible import MADE
    layer = make(kind, D, fdev, dtype, seed=3)
    twin = double_twin(layer)
    g = truth.gen(100 + B + D)
    x0 = torch.randn(B, D, generator=g, dtype=torch.float64)
    gy0 = torch.randn(B, D, generator=g, dtype=torch.float64)
    for reverse in (False, True):
        for p in list(layer.parameters()) + list(twin.parameters()):
            p.grad = None
            # MADE's inverse with grad is the reference's op sequence, which writes x[:, i] in place between the passes: as
            # there, its backward reaches the input but not the weights (the saved x has been overwritten)
            p.requires_grad_(not (reverse and isinstance(layer, MADE)))
        # a non-leaf input (Scaling works in place): x = 1 * leaf
        leaf = x0.to(dtype).to(fdev).detach().clone().requires_grad_(True)
        rleaf = x0.to(dtype).double().detach().clone().requires_grad_(True)
        y, ld = layer(leaf * 1.0, reverse=reverse)
        ry, rld = ref_forward(twin, rleaf * 1.0, reverse)
        close(y, ry, dtype, "value")
        assert (ld is None) == (rld is None)
        loss, rloss = (y * gy0.to(dtype).to(fdev)).sum(), (ry * gy0.to(dtype).double()).sum()
        if ld is not None:
            close(ld, rld, dtype, "log-det")
            assert ld.shape == rld.shape
            loss, rloss = loss + 0.7 * ld.sum(), rloss + 0.7 * rld.sum()
        loss.backward()
        rloss.backward()
        close(leaf.grad, rleaf.grad, dtype, "grad of the input")
        named, rnamed = dict(layer.named_parameters()), dict(twin.named_parameters())
        assert set(named) == set(rnamed)
        for n, p in named.items():
            if rnamed[n].grad is None:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, n
            else:
                assert p.grad is not None and p.grad.shape == p.shape, n
                close(p.grad, rnamed[n].grad, dtype, "grad of " + n)
    if kind in ("maskcoupling_nonbinary", "made_tanh"):
        # values and gradients only: with a mask that is not 0 / 1 the coupling is not a bijection, and MADE's inverse visits the
        # columns `for i in input_degrees` (made.py:117), which is the order of increasing degree only for the sequential order
        return
    # forward, then reverse=True, recovers the input
    with torch.no_grad():
        x = x0.to(dtype).to(fdev)
        y, _ = layer(x.clone())
        back, _ = layer(y.clone(), reverse=True)
        close(back, x, dtype, "round trip")


# ------------------------------------------------------------------------------------------------ interface
def test_import_forms_and_defaults():
    import inspect
    import zhusuan.invertible as inv
    from zhusuan.invertible import (RevNet, get_coupling_mask, MaskCoupling, Coupling, Scaling, RevSequential,  # noqa: F401
                                    MaskedLinear, MADE)
    from zhusuan.invertible.base import RevNet as R2
    from zhusuan.invertible.coupling import MaskCoupling as M2, get_coupling_mask as g2, Coupling as C2, RevSequential as S3  # noqa: F401
    from zhusuan.invertible.scaling import Scaling as S2
    from zhusuan.invertible.sequential import RevSequential as Q2
    from zhusuan.invertible.made import MADE as D2, MaskedLinear as L2
    assert (R2, M2, S2, Q2, D2, L2) == (RevNet, MaskCoupling, Scaling, RevSequential, MADE, MaskedLinear) and g2 is get_coupling_mask
    assert inv.RevNet is RevNet

    def sig(f):
        return [(n, p.default) for n, p in inspect.signature(f).parameters.items() if n != "self"]
    E = inspect.Parameter.empty
    assert sig(get_coupling_mask) == [("n_dim", E), ("n_channel", E), ("n_mask", E), ("split_type", "OddEven"), ("dtype", torch.float32)]
    assert sig(MaskCoupling.__init__) == [("in_out_dim", -1), ("mid_dim", -1), ("hidden", -1), ("mask", None), ("inner_nn", None)]
    assert sig(Coupling.__init__) == [("in_out_dim", E), ("mid_dim", E), ("hidden", E), ("mask_config", E)]
    assert sig(Scaling.__init__) == [("dim", E)]
    assert sig(RevSequential.__init__) == [("layers", E)]
    assert sig(MaskedLinear.__init__) == [("input_size", E), ("n_outputs", E), ("mask", E), ("cond_label_size", None)]
    assert sig(MADE.__init__) == [("input_size", E), ("hidden_size", E), ("n_hidden", E), ("cond_label_size", None),
                                  ("input_order", "sequential"), ("input_degrees", None), ("activation", "relu")]
    assert sig(MADE.create_mask) == [("input_size", E), ("hidden_size", E), ("n_hidden", E), ("input_order", "sequential"),
                                     ("input_degrees", None)]
    assert [n for n, _ in sig(RevNet.forward)] == ["inputs", "reverse", "kwargs"]
    with pytest.raises(NotImplementedError):
        RevNet()._forward(1)
    with pytest.raises(NotImplementedError):
        RevNet()(1, reverse=True)
    with pytest.raises(ValueError):
        MADE(3, 4, 1, activation="gelu")
    with pytest.raises(NotImplementedError):
        MADE.create_mask(3, 4, 1, input_order="other")
    with pytest.raises(NotImplementedError):
        get_coupling_mask(4, 2, 1)


def test_state_dict_keys_and_shapes():
    from zhusuan.invertible import MaskCoupling, Coupling, Scaling, RevSequential, MADE, get_coupling_mask

    def shapes(m):
        return [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    mc = MaskCoupling(6, 5, 2, get_coupling_mask(6, 1, 1)[0])
    assert shapes(mc) == [("nn.0.weight", (5, 6)), ("nn.0.bias", (5,)), ("nn.2.weight", (5, 5)), ("nn.2.bias", (5,)),
                          ("nn.4.weight", (6, 5)), ("nn.4.bias", (6,))]
    assert "mask" not in dict(mc.named_buffers()) and isinstance(mc.mask, torch.Tensor)          # a plain attribute
    inner = nn.Linear(6, 6)
    assert MaskCoupling(mask=mc.mask, inner_nn=inner).nn is inner
    c = Coupling(6, 5, 3, 1)
    assert shapes(c) == [("in_block.0.weight", (5, 3)), ("in_block.0.bias", (5,)), ("mid_block.0.0.weight", (5, 5)),
                         ("mid_block.0.0.bias", (5,)), ("mid_block.1.0.weight", (5, 5)), ("mid_block.1.0.bias", (5,)),
                         ("out_block.weight", (3, 5)), ("out_block.bias", (3,))]
    assert shapes(Scaling(6)) == [("log_scale", (1, 6))]
    assert float(Scaling(6).log_scale.detach().abs().max()) == 0.0 and Scaling(6).log_scale.requires_grad
    seq = RevSequential([mc, Scaling(6)])
    assert [k for k, _ in shapes(seq)] == ["layers.0.nn.0.weight", "layers.0.nn.0.bias", "layers.0.nn.2.weight", "layers.0.nn.2.bias",
                                          "layers.0.nn.4.weight", "layers.0.nn.4.bias", "layers.1.log_scale"]
    m = MADE(4, 7, 2, cond_label_size=3)
    assert shapes(m) == [("base_dist_mean", (4,)), ("base_dist_var", (4,)), ("net_input.weight", (7, 4)), ("net_input.bias", (7,)),
                         ("net_input.cond_weight", (7, 3)), ("net_input.mask", (7, 4)), ("net.1.weight", (7, 7)), ("net.1.bias", (7,)),
                         ("net.1.mask", (7, 7)), ("net.3.weight", (7, 7)), ("net.3.bias", (7,)), ("net.3.mask", (7, 7)),
                         ("net.5.weight", (8, 7)), ("net.5.bias", (8,)), ("net.5.mask", (8, 7))]
    assert sorted(dict(m.named_buffers())) == ["base_dist_mean", "base_dist_var", "net.1.mask", "net.3.mask", "net.5.mask", "net_input.mask"]
    m2 = MADE(4, 7, 2, cond_label_size=3)
    m2.load_state_dict(m.state_dict(), strict=True)
    with pytest.raises(AssertionError):
        RevSequential([nn.Linear(2, 2)])


def test_coupling_masks():
    from zhusuan.invertible import get_coupling_mask
    odd = get_coupling_mask(10, 1, 3)
    assert [m.tolist() for m in odd] == [[0., 1.] * 5, [1., 0.] * 5, [0., 1.] * 5]
    half = get_coupling_mask(10, 1, 2, "Half")
    assert [m.tolist() for m in half] == [[0.] * 5 + [1.] * 5, [1.] * 5 + [0.] * 5]
    assert get_coupling_mask(7, 1, 1, "Half")[0].tolist() == [0.] * 3 + [1.] * 4
    torch.manual_seed(0)
    rh = get_coupling_mask(10, 1, 2, "RandomHalf")
    assert set(rh[0].tolist()) <= {0., 1.} and torch.equal(rh[1], 1. - rh[0])
    for ms in (odd, half, rh):
        assert all(m.dtype == torch.float32 and m.device.type == "cpu" and m.shape == (10,) for m in ms)
    assert get_coupling_mask(4, 1, 1, dtype=torch.float64)[0].dtype == torch.float64
    assert get_coupling_mask(4, 1, 2, "Unknown") == []


def test_made_masks():
    from zhusuan.invertible import MADE
    masks, deg = MADE.create_mask(4, 5, 1)
    assert deg.tolist() == [0, 1, 2, 3] and [tuple(m.shape) for m in masks] == [(5, 4), (5, 5), (4, 5)]
    hid = [0, 1, 2, 0, 1]
    assert masks[0].tolist() == [[float(h >= d) for d in range(4)] for h in hid]
    assert masks[1].tolist() == [[float(a >= b) for b in hid] for a in hid]
    assert masks[2].tolist() == [[float(o - 1 >= h) for h in hid] for o in range(4)]
    assert all(m.dtype == torch.float32 for m in masks)
    _, deg2 = MADE.create_mask(4, 5, 1, input_degrees=torch.tensor([3, 2, 1, 0]))
    assert deg2.tolist() == [3, 2, 1, 0]
    # random order: only the autoregressive property -- output i must not depend on input j unless degree[j] < degree[i].
    # (With the input degrees given, as a stack of MADEs gives them: when create_mask draws them itself it draws the output
    # degrees independently of them, made.py:95, and the masks of a single such layer imply no ordering of the inputs.)
    torch.manual_seed(5)
    masks, deg = MADE.create_mask(5, 9, 2, input_order="random", input_degrees=torch.randperm(5))
    assert sorted(deg.tolist()) == [0, 1, 2, 3, 4]
    own, _ = MADE.create_mask(5, 9, 2, input_order="random")
    assert [tuple(m.shape) for m in own] == [(9, 5), (9, 9), (9, 9), (5, 9)] and all(set(m.flatten().tolist()) <= {0., 1.} for m in own)
    conn = masks[0]
    for m in masks[1:]:
        conn = m @ conn
    for i in range(5):
        for j in range(5):
            if deg[j] >= deg[i]:
                assert float(conn[i, j]) == 0.0, (i, j)


# ------------------------------------------------------------------------------------------------ conventions
def test_scaling_is_in_place_and_refuses_a_leaf(fdev):
    from zhusuan.invertible import Scaling
    sc = Scaling(6).to(fdev)
    with torch.no_grad():
        sc.log_scale.copy_(torch.linspace(-1, 1, 6))
    x = torch.rand(2, 6, device=fdev)
    x0 = x.clone()
    y, ld = sc(x)
    assert y is x and ld.shape == () and ld.dim() == 0
    close(x, x0 * torch.exp(sc.log_scale.detach()), torch.float32)
    back, ld2 = sc(y, reverse=True)
    assert back is x and ld2.shape == ()
    close(x, x0, torch.float32)
    assert float(ld2.detach()) == float(ld.detach())          # sum(log_scale) either way, as in the reference
    with pytest.raises(RuntimeError):
        sc(torch.rand(2, 6, device=fdev, requires_grad=True))


def test_coupling_refuses_an_odd_width_and_log_det_conventions(fdev):
    from zhusuan.invertible import Coupling, MaskCoupling, RevSequential, MADE, get_coupling_mask
    with pytest.raises(RuntimeError):
        Coupling(7, 8, 2, 1).to(fdev)(torch.rand(2, 7, device=fdev))
    x = torch.rand(3, 6, device=fdev)
    mc = MaskCoupling(6, 4, 1, get_coupling_mask(6, 1, 1)[0]).to(fdev)
    assert mc(x)[1] is None and mc(x, reverse=True)[1] is None
    c = Coupling(6, 4, 1, 0).to(fdev)
    assert c(x)[1] is None and c(x, reverse=True)[1] is None
    seq = RevSequential([mc, c])
    for rev in (False, True):
        ld = seq(x, reverse=rev)[1]
        assert isinstance(ld, torch.Tensor) and ld.shape == () and float(ld) == 0.0
    made = MADE(6, 8, 1).to(fdev)
    u, ld = made(x)
    assert ld.shape == (3, 6)
    with torch.no_grad():
        xr, la = made(u, reverse=True)
    assert la.shape == (3, 6)
    close(xr, x, torch.float32)
    close(la, -ld, torch.float32)
    # reverse=True walks the list backwards
    order = []

    class Tap(MaskCoupling):
        def _inverse(self, y, **kw):
            order.append(self.tag)
            return super()._inverse(y, **kw)
    taps = []
    for i in range(3):
        t = Tap(6, 4, 1, get_coupling_mask(6, 1, 1)[0]).to(fdev)
        t.tag = i
        taps.append(t)
    RevSequential(taps)(x, reverse=True)
    assert order == [2, 1, 0]


def test_launch_budget(fdev):
    from zhusuan.invertible import Coupling, MaskCoupling, Scaling, MADE, get_coupling_mask
    x = torch.rand(4, 6, device=fdev)

    def used(c):
        return {k: v for k, v in c.items() if v}
    for layer, fwd, bwd in [
            (MaskCoupling(6, 5, 2, get_coupling_mask(6, 1, 1)[0]), {"split": 1, "merge": 1}, {"split_bwd": 1, "merge_bwd": 1}),
            (Coupling(6, 5, 2, 1), {"split": 1, "merge": 1}, {"split_bwd": 1, "merge_bwd": 1}),
            (Scaling(6), {"scale_fwd": 1}, {"scale_bwd": 1}),
            (MADE(6, 5, 1), {"made_fwd": 1}, {"made_bwd": 1})]:
        layer = layer.to(fdev)
        for reverse in ((False, True) if not isinstance(layer, MADE) else (False,)):
            leaf = x.clone().requires_grad_(True)
            with flow_host.count_launches() as c:
                y, ld = layer(leaf * 1.0, reverse=reverse)
            assert used(c) == fwd, (type(layer).__name__, reverse, used(c))
            loss = y.sum() if ld is None else y.sum() + ld.sum()
            with flow_host.count_launches() as c:
                loss.backward()
            assert used(c) == bwd, (type(layer).__name__, reverse, used(c))


def test_made_inverse_paths(fdev):
    from zhusuan.invertible import MADE
    torch.manual_seed(2)
    made = MADE(5, 8, 2, input_order="random", input_degrees=torch.randperm(5)).to(fdev)
    u = torch.randn(3, 5, device=fdev)
    with flow_host.count_launches() as c, torch.no_grad():
        x1, la1 = made(u, reverse=True)
    assert c["made_inv_col"] == 5 and sum(c.values()) == 5
    for p in made.parameters():
        p.requires_grad_(False)
    with flow_host.count_launches() as c:
        x1b, _ = made(u, reverse=True)                  # grad mode on, nothing requires grad: the column kernel
    assert c["made_inv_col"] == 5 and torch.equal(x1b, x1)
    for p in made.parameters():
        p.requires_grad_(True)
    with flow_host.count_launches() as c:
        x2, la2 = made(u, reverse=True)                 # the reference's op sequence, tracked by autograd
    assert sum(c.values()) == 0 and x2.requires_grad
    close(x2, x1, torch.float32)
    close(la2, la1, torch.float32)
    for p in made.parameters():
        p.requires_grad_(False)
    ug = u.clone().requires_grad_(True)
    with flow_host.count_launches() as c:
        x3, _ = made(ug, reverse=True)
    assert sum(c.values()) == 0
    x3.sum().backward()
    assert ug.grad is not None and bool(torch.isfinite(ug.grad).all())
    # the masked weights are formed once per call and handed to every pass
    from zhusuan.invertible import MaskedLinear
    seen, formed = [], []
    orig_forward, orig_weights = MaskedLinear.forward, MADE._masked_weights

    def forward(self, x, cond_y=None, masked_weight=None):
        seen.append(masked_weight is not None)
        return orig_forward(self, x, cond_y, masked_weight)

    def weights(self):
        formed.append(1)
        return orig_weights(self)
    MaskedLinear.forward, MADE._masked_weights = forward, weights
    try:
        with torch.no_grad():
            made(u, reverse=True)
    finally:
        MaskedLinear.forward, MADE._masked_weights = orig_forward, orig_weights
    assert len(formed) == 1 and len(seen) == 4 * 5 and all(seen)          # four MaskedLinear layers, five passes


def test_dtype_device_and_layout_rules(fdev):
    from zhusuan.invertible import MaskCoupling, Scaling, Coupling, MADE, get_coupling_mask
    mc = MaskCoupling(6, 4, 1, get_coupling_mask(6, 1, 1)[0]).to(fdev)
    for layer in (mc, Scaling(6).to(fdev), Coupling(6, 4, 1, 0).to(fdev), MADE(6, 4, 1).to(fdev)):
        for bad in (torch.float16, torch.int64):
            with pytest.raises(RuntimeError, match=str(bad).replace("torch.", "")):
                layer(torch.ones(2, 6, device=fdev).to(bad))
    # a non-contiguous input is made contiguous by the host layer
    base = torch.rand(6, 2, device=fdev)
    y, _ = mc(base.t())
    y2, _ = mc(base.t().contiguous())
    assert torch.equal(y, y2)


@pytest.mark.gpu
def test_a_host_tensor_raises_on_the_hip_back_end():
    from zhusuan.invertible import Scaling
    flow_host.uninstall()
    with pytest.raises(RuntimeError, match="no CPU path"):
        Scaling(4)(torch.rand(2, 4) * 1.0)


def test_missing_library_error():
    from zhusuan import _flow_hip
    with pytest.raises(RuntimeError, match="make -C zhusuan-pytorch_amd/csrc flow"):
        _flow_hip.lib("/nonexistent/libzs_flow.so")
    with pytest.raises(RuntimeError, match="There is no CPU fallback"):
        _flow_hip.lib(path="/nonexistent/libzs_flow.so")


@pytest.mark.gpu
def test_graphed_flow_vae_step_replays_equal_eager():
    """A small flow-VAE step (three couplings and a scaling between q and p) captured by GraphedStep and replayed three times
    against eager training of a twin: equal losses and parameters (same kernels, same order, same draws: rtol 2e-6 for
    the GEMMs' possible algorithm difference between eager and captured execution, as tests/test_optim.py)."""
    import numpy as np
    import zhusuan as zs
    from examples import flow_vae
    flow_host.uninstall()
    dev = torch.device("cuda:0")

    def make_model():
        torch.manual_seed(4)
        model = flow_vae.build("NICE", 4, 6, 5, 8, device=dev, mid_dim_flow=6, num_coupling=3, num_hidden_per_coupling=2)
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
