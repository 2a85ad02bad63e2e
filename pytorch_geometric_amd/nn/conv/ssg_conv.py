from typing import Optional

from torch import Tensor

from ..._functions import linear
from ..dense.linear import Linear
from ._hops import HopLayer


class SSGConv(HopLayer):
    r"""Simple spectral graph convolution with the constructor arguments, state-dict keys
    (``lin.weight``, ``lin.bias``), ``repr`` and forward semantics of
    ``torch_geometric.nn.SSGConv`` (torch_geometric/nn/conv/ssg_conv.py:64-122):

    .. math:: X' = \Big(\alpha X + \frac{1 - \alpha}{K} \sum_{k=1}^K \hat A^k X\Big) \Theta

    ``cached=True`` keeps the combined features of the first call.  Fused route (``_hops.py``):
    ``K`` launches forward and ``K`` backward; every launch adds its iterate to the running sum
    in its row epilogue (``HopsFunction`` with ``want_sum``).  Without the cache and with
    ``out_channels < in_channels`` the features are transformed first and propagated at the
    narrower width, as in :class:`SGConv`.  Generic route: the reference's loop."""

    def __init__(self, in_channels: int, out_channels: int, alpha: float, K: int = 1,
                 cached: bool = False, add_self_loops: bool = True, bias: bool = True, **kwargs):
        super().__init__(**kwargs)
        self.in_channels, self.out_channels = in_channels, out_channels
        self.alpha, self.K = alpha, K
        self.cached, self.add_self_loops = cached, add_self_loops
        self._cached_h = None
        self.lin = Linear(in_channels, out_channels, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        super().reset_parameters()
        self.lin.reset_parameters()
        self._cached_h = None

    def _combine(self, graph, x: Tensor, edge_weight: Optional[Tensor]) -> Tensor:
        if self.K == 0:
            return x * self.alpha
        return self._steps(graph, x, edge_weight, self.K, d0=self.alpha,
                           d=(1 - self.alpha) / self.K, want_sum=True)[1]

    def forward(self, x: Tensor, edge_index, edge_weight: Optional[Tensor] = None) -> Tensor:
        if self._cached_h is not None:
            return self.lin(self._cached_h.detach())
        edge_index, edge_weight = self._gcn_norm(x, edge_index, edge_weight, self.add_self_loops)
        if self.hop_route(x, edge_index, edge_weight) == 'fused':
            graph = self._graph(x, edge_index)
            if not self.cached and self.out_channels < self.in_channels:
                out = self._combine(graph, linear(x, self.lin.weight), edge_weight)
                return out if self.lin.bias is None else out + self.lin.bias
            h = self._combine(graph, x, edge_weight)
        else:
            h = x * self.alpha
            for _ in range(self.K):
                x = self.propagate(edge_index, x=x, edge_weight=edge_weight)
                h = h + (1 - self.alpha) / self.K * x
        if self.cached:
            self._cached_h = h
        return self.lin(h)

    def __repr__(self) -> str:
        return (f'{self.__class__.__name__}({self.in_channels}, '
                f'{self.out_channels}, K={self.K}, alpha={self.alpha})')
