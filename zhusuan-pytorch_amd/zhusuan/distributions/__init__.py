"""Distributions of the variational-inference hot path (Normal, Bernoulli) and, as the first widening step
(SURVEY.md 8f rank 4), the reference's two other hand-written samplers (Logistic, Uniform).

The reference also ships Beta, Gamma, Laplace, StudentT, Poisson, Exponential (thin wrappers of
torch.distributions, zhusuan/distributions/__init__.py:3-13): off the hot path named by BASELINE.json, kept as equally thin
pass-throughs (``torch_families.py``: plain torch ops, no kernels) so that existing model code keeps working.  FlowDistribution
(flow_distribution.py) wraps a base distribution and a ``zhusuan.invertible`` network; its log-density tail runs on the flow
kernels of include/zs_flow.h.

Categorical / OnehotCategorical and their relaxations ExpConcrete / Concrete (upstream ZhuSuan has them, the PyTorch reference
dropped them) run on the categorical kernels of include/zs_cat.h, a library of its own that is loaded on their first use;
MultivariateNormalCholesky (the same history) runs on the triangular kernels of include/zs_mvn.h, likewise."""
from .base import Distribution
from .normal import Normal
from .bernoulli import Bernoulli
from .logistic import Logistic
from .uniform import Uniform
from .torch_families import Beta, Exponential, Gamma, Laplace, Poisson, StudentT, FlowDistribution
from .categorical import Categorical, OnehotCategorical, Discrete, OnehotDiscrete
from .concrete import ExpConcrete, Concrete, ExpGumbelSoftmax, GumbelSoftmax
from .multivariate import MultivariateNormalCholesky

__all__ = ['Distribution', 'Normal', 'Bernoulli', 'Logistic', 'Uniform',
           # torch.distributions pass-throughs (no kernels) and the flow-defined distribution:
           'Beta', 'Exponential', 'Gamma', 'Laplace', 'Poisson', 'StudentT', 'FlowDistribution',
           # the categorical kernels (include/zs_cat.h):
           'Categorical', 'OnehotCategorical', 'Discrete', 'OnehotDiscrete', 'ExpConcrete', 'Concrete', 'ExpGumbelSoftmax',
           'GumbelSoftmax',
           # the triangular kernels (include/zs_mvn.h):
           'MultivariateNormalCholesky']
