from typing import Optional

from torch import Tensor

from ..._functions import linear
from ..dense.linear import Linear
from ._hops import HopLayer


class SGConv(HopLayer):
    r"""Simple graph convolution ``X' = \hat A^K X \Theta`` with the constructor arguments,
    state-dict keys (``lin.weight``, ``lin.bias``), ``repr`` and forward semantics of
    ``torch_geometric.nn.SGConv`` (torch_geometric/nn/conv/sg_conv.py:56-111).  ``cached=True``
    keeps the propagated features ``\hat A^K X`` of the first call.

    Fused route (``_hops.py``): ``K`` launches forward and ``K`` backward (``HopsFunction``).
    Without the cache and with ``out_channels < in_channels`` the features are transformed first
    and propagated at the narrower width — ``(\hat A^K X) W = \hat A^K (X W)`` for a linear
    message flow; ``cached=True`` keeps the reference's order, since the cache holds
    ``\hat A^K X``.  Generic route: the reference's loop."""

    def __init__(self, in_channels: int, out_channels: int, K: int = 1, cached: bool = False,
                 add_self_loops: bool = True, bias: bool = True, **kwargs):
        super().__init__(**kwargs)
        self.in_channels, self.out_channels, self.K = in_channels, out_channels, K
        self.cached, self.add_self_loops = cached, add_self_loops
        self._cached_x = None
        self.lin = Linear(in_channels, out_channels, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        super().reset_parameters()
        self.lin.reset_parameters()
        self._cached_x = None

    def forward(self, x: Tensor, edge_index, edge_weight: Optional[Tensor] = None) -> Tensor:
        if self._cached_x is not None:
            return self.lin(self._cached_x.detach())
        edge_index, edge_weight = self._gcn_norm(x, edge_index, edge_weight, self.add_self_loops)
        if self.hop_route(x, edge_index, edge_weight) == 'fused':
            graph = self._graph(x, edge_index)
            if not self.cached and self.out_channels < self.in_channels:
                out = self._steps(graph, linear(x, self.lin.weight), edge_weight, self.K)
                return out if self.lin.bias is None else out + self.lin.bias
            x = self._steps(graph, x, edge_weight, self.K)
            if self.cached and self.K > 0:
                self._cached_x = x
            return self.lin(x)
        for _ in range(self.K):
            x = self.propagate(edge_index, x=x, edge_weight=edge_weight)
            if self.cached:
                self._cached_x = x
        return self.lin(x)

    def __repr__(self) -> str:
        return (f'{self.__class__.__name__}({self.in_channels}, '
                f'{self.out_channels}, K={self.K})')
