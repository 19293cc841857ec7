"""Invertible (normalising-flow) layers on the kernels of include/zs_flow.h: the reference's ``zhusuan.invertible``."""
from .base import *
from .coupling import *
from .scaling import *
from .sequential import *
from .made import *
