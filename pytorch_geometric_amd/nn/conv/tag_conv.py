from typing import Optional

import torch
from torch import Tensor

from ..._functions import linear
from ..dense.linear import Linear
from ..inits import zeros
from ._hops import HopLayer


class TAGConv(HopLayer):
    r"""Topology-adaptive graph convolution ``X' = \sum_{k=0}^K \hat A^k X W_k`` (no self-loops
    in ``\hat A``) with the constructor arguments, state-dict keys (``lins.<k>.weight``,
    ``bias``), ``repr`` and forward semantics of ``torch_geometric.nn.TAGConv``
    (torch_geometric/nn/conv/tag_conv.py:45-106).

    Fused route (``_hops.py``): ``K`` launches and ``K + 1`` transforms.  With ``out_channels <
    in_channels`` the sum is evaluated in Horner form at the narrower width, ``t_K = X W_K``,
    ``t_k = \hat A t_{k+1} + X W_k``: all ``X W_k`` come from ONE dense product with the stacked
    weights, and a launch reads its block of that plane in place as the epilogue term.  Generic
    route: the reference's loop."""

    def __init__(self, in_channels: int, out_channels: int, K: int = 3, bias: bool = True,
                 normalize: bool = True, **kwargs):
        super().__init__(**kwargs)
        self.in_channels, self.out_channels, self.K = in_channels, out_channels, K
        self.normalize = normalize
        self.lins = torch.nn.ModuleList(
            [Linear(in_channels, out_channels, bias=False) for _ in range(K + 1)])
        if bias:
            self.bias = torch.nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        super().reset_parameters()
        for lin in self.lins:
            lin.reset_parameters()
        zeros(self.bias)

    def forward(self, x: Tensor, edge_index, edge_weight: Optional[Tensor] = None) -> Tensor:
        if self.normalize:
            edge_index, edge_weight = self._gcn_norm(x, edge_index, edge_weight, False)
        if self.hop_route(x, edge_index, edge_weight) == 'fused':
            graph = self._graph(x, edge_index)
            if self.out_channels < self.in_channels:
                stacked = torch.cat([lin.weight for lin in self.lins], dim=0)
                blocks = linear(x, stacked).split(self.out_channels, dim=1)
                out = blocks[self.K]
                for k in range(self.K - 1, -1, -1):
                    out = self._step(graph, out, edge_weight, 1.0, z=blocks[k], c=1.0)
            else:
                out = self.lins[0](x)
                for lin in self.lins[1:]:
                    x = self._step(graph, x, edge_weight)
                    out = out + lin(x)
        else:
            out = self.lins[0](x)
            for lin in self.lins[1:]:
                x = self.propagate(edge_index, x=x, edge_weight=edge_weight)
                out = out + lin(x)
        if self.bias is not None:
            out = out + self.bias
        return out

    def __repr__(self) -> str:
        return (f'{self.__class__.__name__}({self.in_channels}, '
                f'{self.out_channels}, K={self.K})')
