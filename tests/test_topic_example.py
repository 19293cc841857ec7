"""examples/lntm_mcem.py, the logistic-normal topic model the reference left unfinished, at a tiny size on the GPU."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_example_runs_at_a_tiny_size():
    from examples import lntm_mcem
    r = lntm_mcem.run(n_chains=2, n_docs=6, n_topics=3, n_words=40, n_rounds=3, device="cuda:0")
    assert len(r["per_word_ll"]) == 3 and all(math.isfinite(v) and v < 0 for v in r["per_word_ll"])
    assert 0.0 < r["acceptance"] <= 1.0 and math.isfinite(r["step_size"]) and r["step_size"] > 0
    shapes = dict(beta=(3, 40), eta=(2, 6, 3), eta_mean=(3,), eta_logstd=(3,))
    for name, shape in shapes.items():
        assert tuple(r[name].shape) == shape and r[name].device.type == "cuda" and bool(torch.isfinite(r[name]).all()), name
