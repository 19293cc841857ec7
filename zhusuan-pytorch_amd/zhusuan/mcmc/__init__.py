"""Stochastic-gradient MCMC samplers (zhusuan/mcmc/__init__.py:1-2 of the reference).  Not imported by ``import zhusuan``,
as with the reference; the kernel library behind it (lib/libzs_mcmc.so) is loaded on the first update.  ``HMC`` (no counterpart in the reference, which only carries its intended call, commented out, in
test/mcmc/test_mcmc.py) runs on a library of its own, lib/libzs_hmc.so, loaded on its first iteration."""
from .SGLD import *
from .SGHMC import *
from .HMC import *
