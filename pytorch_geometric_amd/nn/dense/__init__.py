from .linear import HeteroDictLinear, HeteroLinear, Linear
