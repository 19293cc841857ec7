"""examples/bnn_matvar.py, the BNN regression example with a matrix-variate posterior over each layer's weights, at a tiny size on
the GPU."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_example_runs_at_a_tiny_size():
    from examples import bnn_matvar
    r = bnn_matvar.run(layer_sizes=(5, 17, 1), n_particles=3, batch=12, steps=4, device="cuda:0")
    assert len(r["losses"]) == 4 and all(math.isfinite(v) for v in r["losses"])
    q = r["model"].variational
    assert q.structured == [True, True]
    paths = [n.dist.last_path["path"] for n in q.nodes.values()]
    assert len(paths) == 2 and all(p.startswith("M1 zs_matvar_sample_logprob") for p in paths)
    for i, (n, p) in enumerate(((6, 17), (18, 1))):          # the gradients reach the mean and both factors of every layer
        for prm, shape in ((q.w_means[i], (n, p)), (q.w_rows[i], (n, n)), (q.w_cols[i], (p, p))):
            assert tuple(prm.grad.shape) == shape and bool(torch.isfinite(prm.grad).all()) and float(prm.grad.abs().max()) > 0
