"""TEST INFRASTRUCTURE shared by the satellite product tests: the suite's accuracy rule against a float64 truth, and the seeding
helpers."""
import math

import torch

import host_backend


def held_to_the_rule(tag, items, worst=None):
    """The suite's rule for every ``(name, got, float32 restatement, float64 truth)`` of ``items``: the error against the float64
    truth is at most 16 x the float32 restatement's own distance from it.  Returns the worst multiple err / dist seen (0 where
    both are 0, inf where only dist is) and keeps the maximum per ``(tag, name)`` in the dict ``worst``, if one is given."""
    top = 0.0
    for name, got, f32, f64 in items:
        got, f32, f64 = (t.detach().cpu().double() for t in (got, f32, f64))
        dist = float((f32 - f64).abs().max())
        err = float((got - f64).abs().max())
        multiple = err / dist if dist > 0 else (0.0 if err == 0 else math.inf)
        print("%s %s: error %.3e, the float32 restatement's own distance %.3e (%.2f x)" % (tag, name, err, dist, multiple))
        if worst is not None:
            worst[(tag, name)] = max(worst.get((tag, name), 0.0), multiple)
        top = max(top, multiple)
        assert err <= 16 * dist, (tag, name, err, dist)
    return top


def gen(seed):
    return torch.Generator().manual_seed(seed)


def seed_all(s, dev=None):
    """Seeds torch and the host back-end's Philox pair; given a GPU device, torch and that device's generator instead."""
    torch.manual_seed(s)
    if dev is not None and dev.type != "cpu":
        torch.cuda.manual_seed(s)
    else:
        host_backend.manual_seed(s)
