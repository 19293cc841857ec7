"""Variational objectives of the hot path: the evidence lower bound (sgvb / reinforce estimators) and the
importance-weighted bound (sgvb / vimco) -- the import surface of the reference's ``zhusuan.variational`` package -- and the
inclusive KL divergence (upstream's ``klpq``: importance / rws), which the reference does not have."""
from .importance_weighted_objective import ImportanceWeightedObjective
from .elbo import EvidenceLowerBoundObjective, ELBO
from .inclusive_kl import InclusiveKLObjective, KLpq

__all__ = ['ELBO', 'EvidenceLowerBoundObjective', 'ImportanceWeightedObjective', 'InclusiveKLObjective', 'KLpq']
