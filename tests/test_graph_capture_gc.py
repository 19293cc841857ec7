"""``zhusuan.graph._capture``: every graph capture of GraphedStep / GraphedStages starts with Python's dead cycles collected and runs
with the cyclic collector off.  torch does not collect before a capture by default (``torch.compiler.config.force_cudagraph_gc``),
and a generational collection that fires inside a capture and frees a dead cycle holding HIP resources aborted the GPU suite.
The capture itself is replaced by a stand-in here, so the test needs no GPU."""
import contextlib
import gc
import weakref

import pytest
import torch


class _Node(object):
    pass


@pytest.mark.parametrize("enabled_before", [True, False])
def test_capture_collects_first_and_keeps_the_collector_off_until_it_ends(monkeypatch, enabled_before):
    from zhusuan import graph
    seen = {}

    @contextlib.contextmanager
    def stand_in(g, **kwargs):
        seen["enter"] = (gc.isenabled(), dead() is None, g, kwargs)
        yield
        seen["exit"] = gc.isenabled()
    monkeypatch.setattr(torch.cuda, "graph", stand_in)
    a, b = _Node(), _Node()
    a.other, b.other = b, a          # a dead cycle, as an earlier GraphedStep is (its closures refer to it)
    dead = weakref.ref(a)
    was = gc.isenabled()
    gc.disable()                     # (so that only _capture's own collection can free the cycle)
    del a, b
    assert dead() is not None
    try:
        if enabled_before:
            gc.enable()
        with graph._capture("g", pool="p"):
            seen["inside"] = gc.isenabled()
        assert seen["enter"] == (False, True, "g", {"capture_error_mode": "thread_local", "pool": "p"})
        assert seen["inside"] is False and seen["exit"] is False
        assert gc.isenabled() is enabled_before          # put back as it was found
        with pytest.raises(KeyError):                    # ... also when the captured step raises
            with graph._capture("g"):
                raise KeyError("step")
        assert gc.isenabled() is enabled_before
    finally:
        (gc.enable if was else gc.disable)()


def test_every_capture_of_the_module_goes_through_it():
    import inspect

    from zhusuan import graph
    src = inspect.getsource(graph)
    assert src.count("with torch.cuda.graph(") == 1 and src.count("with _capture(") == 5
