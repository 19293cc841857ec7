"""The shared helpers of the product-level tests themselves (tests/host_routing.py, tests/truth.py, tests/reference_runs.py),
against a throw-away module object: no binding, no GPU."""
import sys
import types

import numpy as np
import pytest
import torch

import host_routing
from host_routing import Router, host_only, routed
from reference_runs import same_fixtures
from truth import held_to_the_rule

CPU, CUDA = torch.device("cpu"), torch.device("cuda:0")


@pytest.fixture
def binding(monkeypatch):
    """A module ``toy_binding`` with two functions, and a router that replaces both."""
    m = types.ModuleType("toy_binding")
    m.f = lambda *a, **k: "real f"
    m.g = lambda *a, **k: "real g"
    monkeypatch.setitem(sys.modules, "toy_binding", m)
    return m, Router("toy_binding", {"f": lambda *a, **k: "host f", "g": lambda *a, **k: "host g"})


def test_install_and_uninstall_are_idempotent_and_restore_the_first_originals(binding):
    m, r = binding
    real = m.f, m.g
    r.uninstall()
    assert (m.f, m.g) == real
    r.install()
    r.install()
    assert (m.f(), m.g()) == ("host f", "host g")
    r.uninstall()
    assert (m.f, m.g) == real
    r.uninstall()
    assert (m.f, m.g) == real


def test_recording_restores_what_it_found_when_the_block_raises(binding):
    m, r = binding
    real = m.f, m.g
    with pytest.raises(KeyError):
        with r.recording():
            assert m.f is not real[0]
            raise KeyError("x")
    assert (m.f, m.g) == real
    r.install()
    held = m.f, m.g
    with pytest.raises(KeyError):
        with r.recording():
            raise KeyError("x")
    assert (m.f, m.g) == held
    r.uninstall()
    assert (m.f, m.g) == real


def test_nested_recordings_both_see_a_call_and_count_counts(binding):
    m, r = binding
    with r.recording() as outer:
        m.f(1)
        with r.recording() as inner, r.count() as c:
            assert m.g(2, k=3) == "real g"
        m.f(4)
    assert [(x.name, x.args, x.kwargs) for x in outer] == [("f", (1,), {}), ("g", (2,), {"k": 3}), ("f", (4,), {})]
    assert inner == [("g", (2,), {"k": 3})] and inner[0].name == inner[0][0] == "g"
    assert c == {"f": 0, "g": 1}


def test_recordings_opened_before_and_after_install_see_the_function_that_runs(binding):
    m, r = binding
    real = m.f, m.g
    with r.recording() as before:
        assert m.f() == "real f"
        r.install()
        with r.recording() as after:
            assert m.f() == "host f"
        r.uninstall()
        assert m.g() == "real g"
    assert [c.name for c in before] == ["f", "f", "g"] and [c.name for c in after] == ["f"]
    assert (m.f, m.g) == real
    # an install() inside the block outlives the block; uninstall() then restores the originals
    with r.recording():
        r.install()
    assert m.f() == "host f"
    r.uninstall()
    assert (m.f, m.g) == real


def test_tensors_become_shapes_and_everything_else_passes_through(binding):
    m, r = binding
    t, marker = torch.zeros(2, 3), object()
    with r.recording() as calls:
        m.f(t, 5, None, marker, (t, "s"), terms=[t, [torch.zeros(4), 1.5]], flags={"a": t, "b": True})
    (c,) = calls
    assert c.args == ((2, 3), 5, None, marker, ((2, 3), "s"))
    assert c.kwargs == {"terms": [(2, 3), [(4,), 1.5]], "flags": {"a": (2, 3), "b": True}}


def two_routers(m):
    order = []

    class Noting(Router):
        def uninstall(self):
            if self._saved is not None:
                order.append(self.functions)
            Router.uninstall(self)
    a, b = Noting("toy_binding", {"f": lambda: "host f"}), Noting("toy_binding", {"g": lambda: "host g"})
    return a, b, order


def test_routed_installs_all_on_the_host_and_uninstalls_in_reverse_order_when_the_block_raises(binding):
    m, _ = binding
    real = m.f, m.g
    a, b, order = two_routers(m)
    body = routed(CPU, a, b)
    assert next(body) == CPU and (m.f(), m.g()) == ("host f", "host g")
    with pytest.raises(KeyError):
        body.throw(KeyError("x"))
    assert (m.f, m.g) == real and order == [b.functions, a.functions]


def test_routed_uninstalls_all_on_the_gpu_and_host_undoes_the_main_binding_too(binding):
    m, _ = binding
    real = m.f, m.g
    a, b, order = two_routers(m)
    a.install(), b.install()
    assert next(routed(CUDA, a, b)) == CUDA and (m.f, m.g) == real
    from zhusuan import _hip
    lib = _hip.lib
    with pytest.raises(KeyError):
        with host_routing.host(a, b) as dev:
            assert dev == CPU and (m.f(), m.g()) == ("host f", "host g") and _hip.lib is not lib
            raise KeyError("x")
    assert (m.f, m.g) == real and _hip.lib is lib


def test_dev_fixture_is_found_under_its_name():
    fx = host_routing.dev_fixture("zdev", doc="doc")
    marker = getattr(fx, "_fixture_function_marker", None) or fx._pytestfixturefunction
    assert marker.name == "zdev"


def test_host_only():
    host_only("toy_host", [None, torch.zeros(2), [torch.zeros(1), None, (torch.zeros(3),)]])
    with pytest.raises(RuntimeError, match="tests/toy_host: host restatement installed but tensor is on meta"):
        host_only("toy_host", [torch.zeros(2), [None, torch.zeros(2, device="meta")]])


# ------------------------------------------------------------------------------------------------ truth.held_to_the_rule
def T(*v):
    return torch.tensor(v, dtype=torch.float64)


def test_the_rule_holds_at_sixteen_times_the_distance_and_fails_just_above():
    # dist = 2^-10 exactly; err = 2^-6 = 16 dist exactly
    assert held_to_the_rule("t", [("at", T(1 + 2.0 ** -6), T(1 + 2.0 ** -10), T(1.0))]) == 16.0
    with pytest.raises(AssertionError) as e:
        held_to_the_rule("t", [("above", T(1 + 2.0 ** -6 + 2.0 ** -40), T(1 + 2.0 ** -10), T(1.0))])
    assert "above" in str(e.value)
    assert held_to_the_rule("t", [("same", T(1.0, 2.0), T(1.0, 2.0), T(1.0, 2.0))]) == 0.0
    with pytest.raises(AssertionError):
        held_to_the_rule("t", [("no room", T(1 + 2.0 ** -50), T(1.0), T(1.0))])
    with pytest.raises(AssertionError):
        held_to_the_rule("t", [("nan", T(1.0, float("nan")), T(1.0 + 2.0 ** -10, 2.0), T(1.0, 2.0))])


def test_the_rule_keeps_the_maximum_in_the_worst_dict():
    worst = {}
    f32, f64 = T(1 + 2.0 ** -10), T(1.0)
    assert held_to_the_rule("t", [("a", T(1 + 2.0 ** -8), f32, f64), ("b", T(1 + 2.0 ** -9), f32, f64)], worst) == 4.0
    assert held_to_the_rule("t", [("a", T(1 + 2.0 ** -9), f32, f64)], worst) == 2.0
    assert held_to_the_rule("t", [("b", T(1 + 2.0 ** -7), f32.float(), f64)], worst) == 8.0          # (any dtype, any device)
    assert worst == {("t", "a"): 4.0, ("t", "b"): 8.0}


# ------------------------------------------------------------------------------------------------ reference_runs.same_fixtures
def fixtures(d, **files):
    d.mkdir()
    for name, arrays in files.items():
        np.savez(d / (name + ".npz"), **arrays)
    (d / "notes.txt").write_text("not a fixture")
    return str(d)


def test_same_fixtures(tmp_path):
    one = dict(x=np.arange(3, dtype=np.float32), n=np.array([1, 2]))
    nan = dict(x=np.array([1.0, np.nan]), i=np.array([3]))
    a = fixtures(tmp_path / "a", one=one, two=dict(y=np.zeros((2, 2))))
    assert same_fixtures(a, fixtures(tmp_path / "b", one=one, two=dict(y=np.zeros((2, 2))))) == 3
    for k, (other, why) in enumerate([
            (dict(one=dict(one, x=np.array([0, 1, 3], dtype=np.float32)), two=dict(y=np.zeros((2, 2)))), "value"),
            (dict(one=dict(one, x=np.arange(3, dtype=np.float64)), two=dict(y=np.zeros((2, 2)))), "dtype"),
            (dict(one=dict(x=one["x"]), two=dict(y=np.zeros((2, 2)))), "missing key"),
            (dict(one=one), "missing file")]):
        with pytest.raises(AssertionError):
            same_fixtures(a, fixtures(tmp_path / ("c%d" % k), **other))
        with pytest.raises(AssertionError):
            same_fixtures(str(tmp_path / ("c%d" % k)), a)
    n1, n2 = fixtures(tmp_path / "n1", f=nan), fixtures(tmp_path / "n2", f=nan)
    assert same_fixtures(n1, n2, equal_nan=True) == 2
    with pytest.raises(AssertionError):
        same_fixtures(n1, n2)
