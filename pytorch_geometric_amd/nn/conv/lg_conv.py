from typing import Optional

from torch import Tensor

from ._hops import HopLayer


class LGConv(HopLayer):
    r"""The light graph convolution of LightGCN, ``x_i' = \sum_{j \in N(i)}
    \frac{e_{ji}}{\sqrt{\deg(i) \deg(j)}} x_j``, with the constructor arguments and forward
    semantics of ``torch_geometric.nn.LGConv`` (torch_geometric/nn/conv/lg_conv.py:32-56); the
    layer has no parameters.  Fused route (``_hops.py``): one launch forward and one backward
    (``HopFunction``).  Generic route: ``propagate``.  A single step has no combination for the
    epilogue to absorb, and ``propagate``'s SpMM (compiled autograd node, streamed stores) was 1.5
    to 4 % faster at both shapes measured (profiles/propagate_hops.md): unless ``PYGAMD_FUSE_HOPS``
    says otherwise the layer starts with ``fuse = False``."""

    FUSE_DEFAULT = False

    def __init__(self, normalize: bool = True, **kwargs):
        super().__init__(**kwargs)
        self.normalize = normalize

    def forward(self, x: Tensor, edge_index, edge_weight: Optional[Tensor] = None) -> Tensor:
        if self.normalize:
            edge_index, edge_weight = self._gcn_norm(x, edge_index, edge_weight, False)
        if self.hop_route(x, edge_index, edge_weight) == 'fused':
            return self._step(self._graph(x, edge_index), x, edge_weight)
        return self.propagate(edge_index, x=x, edge_weight=edge_weight)
