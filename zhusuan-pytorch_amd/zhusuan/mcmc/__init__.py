"""Stochastic-gradient MCMC samplers (zhusuan/mcmc/__init__.py:1-2 of the reference).  Not imported by ``import zhusuan``,
as with the reference; the kernel library behind it (lib/libzs_mcmc.so) is loaded on the first update."""
from .SGLD import *
from .SGHMC import *
