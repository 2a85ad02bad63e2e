from math import log
from typing import Optional

import torch
from torch import Tensor
from torch.nn import Parameter

from ..inits import glorot
from ._hops import HopLayer


class GCN2Conv(HopLayer):
    r"""Graph convolution with initial residual and identity mapping (GCNII), with the
    constructor arguments, parameters (``weight1`` and, with ``shared_weights=False``,
    ``weight2``; glorot), ``repr`` and forward semantics of ``torch_geometric.nn.GCN2Conv``
    (torch_geometric/nn/conv/gcn2_conv.py:74-163):

    .. math:: X' = \big((1 - \alpha) \hat A X + \alpha X^{(0)}\big)
              \big((1 - \beta) I + \beta \Theta\big), \qquad \beta = \log(\theta / \ell + 1)

    ``cached=True`` keeps the normalised edge list.  Fused route (``_hops.py``): one launch
    forward and one backward; with shared weights the initial residual is the launch's epilogue
    term, with separate weights ``x_0`` is scaled on its own as in the reference.  The two
    ``addmm`` stay dense products.  Generic route: the reference's sequence."""

    def __init__(self, channels: int, alpha: float, theta: float = None, layer: int = None,
                 shared_weights: bool = True, cached: bool = False, add_self_loops: bool = True,
                 normalize: bool = True, **kwargs):
        super().__init__(**kwargs)
        self.channels, self.alpha, self.beta = channels, alpha, 1.
        if theta is not None or layer is not None:
            assert theta is not None and layer is not None
            self.beta = log(theta / layer + 1)
        self.cached, self.normalize, self.add_self_loops = cached, normalize, add_self_loops
        self._cached_edge_index = None
        self.weight1 = Parameter(torch.empty(channels, channels))
        if shared_weights:
            self.register_parameter('weight2', None)
        else:
            self.weight2 = Parameter(torch.empty(channels, channels))
        self.reset_parameters()

    def reset_parameters(self):
        super().reset_parameters()
        glorot(self.weight1)
        glorot(self.weight2)
        self._cached_edge_index = None

    def forward(self, x: Tensor, x_0: Tensor, edge_index,
                edge_weight: Optional[Tensor] = None) -> Tensor:
        if self.normalize:
            edge_index, edge_weight = self._gcn_norm(x, edge_index, edge_weight,
                                                     self.add_self_loops, '_cached_edge_index')
        fused = (self.hop_route(x, edge_index, edge_weight) == 'fused' and x_0.is_cuda
                 and x_0.dtype == x.dtype and x_0.dim() == 2 and x_0.size(1) == x.size(1)
                 and x_0.size(0) >= x.size(0))
        shared = self.weight2 is None
        if fused:
            graph = self._graph(x, edge_index)
            if shared:
                out = self._step(graph, x, edge_weight, 1 - self.alpha, x_0[:x.size(0)],
                                 self.alpha)
            else:
                x = self._step(graph, x, edge_weight, 1 - self.alpha)
                x_0 = self.alpha * x_0[:x.size(0)]
        else:
            x = self.propagate(edge_index, x=x, edge_weight=edge_weight)
            x = x * (1 - self.alpha)
            x_0 = self.alpha * x_0[:x.size(0)]
            if shared:
                out = x + x_0
        if shared:
            return torch.addmm(out, out, self.weight1, beta=1. - self.beta, alpha=self.beta)
        out = torch.addmm(x, x, self.weight1, beta=1. - self.beta, alpha=self.beta)
        return out + torch.addmm(x_0, x_0, self.weight2, beta=1. - self.beta, alpha=self.beta)

    def __repr__(self) -> str:
        return (f'{self.__class__.__name__}({self.channels}, '
                f'alpha={self.alpha}, beta={self.beta})')
