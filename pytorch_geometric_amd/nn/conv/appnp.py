from typing import Optional

import torch.nn.functional as F
from torch import Tensor

from ._hops import HopLayer


class APPNP(HopLayer):
    r"""Approximate personalised propagation of neural predictions, with the constructor
    arguments, ``repr`` and forward semantics of ``torch_geometric.nn.APPNP``
    (torch_geometric/nn/conv/appnp.py:61-142); the layer has no parameters:

    .. math:: x^{(0)} = x, \qquad x^{(k)} = (1 - \alpha) \hat A x^{(k-1)} + \alpha x^{(0)}

    ``cached=True`` keeps the normalised edge list.  Routes (``_hops.py``): fused — ``K`` launches
    forward and ``K`` backward, the combination with ``x^{(0)}`` being the row epilogue
    (``HopsFunction``, nothing per step is saved); with ``dropout > 0`` in training every step
    draws its own ``F.dropout(edge_weight)`` exactly where the reference does and runs as one
    ``HopFunction``.  Generic: the reference's loop."""

    def __init__(self, K: int, alpha: float, dropout: float = 0., cached: bool = False,
                 add_self_loops: bool = True, normalize: bool = True, **kwargs):
        super().__init__(**kwargs)
        self.K, self.alpha, self.dropout = K, alpha, dropout
        self.cached, self.add_self_loops, self.normalize = cached, add_self_loops, normalize
        self._cached_edge_index = None

    def reset_parameters(self):
        super().reset_parameters()
        self._cached_edge_index = None

    def forward(self, x: Tensor, edge_index, edge_weight: Optional[Tensor] = None) -> Tensor:
        if self.normalize:
            edge_index, edge_weight = self._gcn_norm(x, edge_index, edge_weight,
                                                     self.add_self_loops, '_cached_edge_index')
        drop = self.dropout > 0 and self.training
        if drop:
            assert edge_weight is not None
        if self.hop_route(x, edge_index, edge_weight) == 'fused':
            graph = self._graph(x, edge_index)
            if not drop:
                return self._steps(graph, x, edge_weight, self.K, 1 - self.alpha, self.alpha,
                                   tied=True)
            h = x
            for _ in range(self.K):
                edge_weight = F.dropout(edge_weight, p=self.dropout)
                x = self._step(graph, x, edge_weight, 1 - self.alpha, h, self.alpha)
            return x
        h = x
        for _ in range(self.K):
            if drop:
                edge_weight = F.dropout(edge_weight, p=self.dropout)
            x = self.propagate(edge_index, x=x, edge_weight=edge_weight)
            x = x * (1 - self.alpha)
            x = x + self.alpha * h
        return x

    def __repr__(self) -> str:
        return f'{self.__class__.__name__}(K={self.K}, alpha={self.alpha})'
