"""How the samplers cut their latents into launches: every kernel of zhusuan.mcmc takes a table of at most ``max_tensors``
tensors of one dtype, forming one flat index space."""
import torch


class Chunk(object):
    """The latents of one launch: positions ``idx`` in the sampler's latent list, their shapes and common dtype."""

    def __init__(self, idx, shapes, dtype):
        self.idx = idx
        self.shapes = shapes
        self.dtype = dtype
        self.sizes = [int(torch.Size(s).numel()) for s in shapes]
        self.n = sum(self.sizes)

    def split(self, flat):
        """Views of a flat tensor of ``n`` elements with the latents' shapes, in order."""
        out, a = [], 0
        for s, k in zip(self.shapes, self.sizes):
            out.append(flat[a:a + k].view(s))
            a += k
        return out


def plan_chunks(tensors, key, max_tensors):
    """Yield ``(key(t), indices)`` per launch: the non-empty tensors grouped by ``key`` (groups in order of first appearance,
    tensors in list order), each group cut into runs of at most ``max_tensors``.  The order is part of the samplers' contract:
    Philox call ids are handed out along it."""
    groups = {}
    for i, t in enumerate(tensors):
        if t.numel():
            groups.setdefault(key(t), []).append(i)
    for k, idx in groups.items():
        for a in range(0, len(idx), max_tensors):
            yield k, idx[a:a + max_tensors]
