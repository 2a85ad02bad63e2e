from typing import Callable, Optional, Tuple, Union

import torch
from torch import Tensor

from ..conv import GraphConv
from ._fuse import fuse_default
from .connect import FilterEdges
from .select import SelectTopK
from .topk_pool import HierarchicalPooling


class SAGPooling(HierarchicalPooling):
    r"""Self-attention graph pooling with the constructor arguments, the ``forward`` arguments,
    the six-tuple result ``(x, edge_index, edge_attr, batch, perm, score)``, the parameters
    (``gnn.*``, ``select.weight``) and the ``__repr__`` of ``torch_geometric.nn.SAGPooling``
    (torch_geometric/nn/pool/sag_pool.py:12-150):

    .. math:: \mathbf{y} = \textrm{GNN}(\mathbf{X}, \mathbf{A}), \quad \mathbf{i} =
              \mathrm{top}_k(\mathbf{y}), \quad \mathbf{X}^{\prime} = (\mathbf{X} \odot
              \mathrm{tanh}(\mathbf{y}))_{\mathbf{i}}, \quad \mathbf{A}^{\prime} =
              \mathbf{A}_{\mathbf{i},\mathbf{i}}

    The projection scores come from ``GNN(in_channels, 1, **kwargs)``, a conv layer of this
    package (default :class:`~pytorch_geometric_amd.nn.GraphConv`); selection, scaling and edge
    filter are :class:`TopKPooling`'s, with its routes and its ``fuse`` attribute."""

    def __init__(self, in_channels: int, ratio: Union[float, int] = 0.5,
                 GNN: torch.nn.Module = GraphConv, min_score: Optional[float] = None,
                 multiplier: float = 1.0, nonlinearity: Union[str, Callable] = 'tanh', **kwargs):
        super().__init__()
        self.in_channels = in_channels
        self.ratio = ratio
        self.min_score = min_score
        self.multiplier = multiplier
        self.gnn = GNN(in_channels, 1, **kwargs)
        self.select = SelectTopK(1, ratio, min_score, nonlinearity)
        self.connect = FilterEdges()
        self.fuse = fuse_default('SAGPooling')
        self.reset_parameters()

    def reset_parameters(self):
        self.gnn.reset_parameters()
        self.select.reset_parameters()

    def forward(self, x: Tensor, edge_index: Tensor, edge_attr: Optional[Tensor] = None,
                batch: Optional[Tensor] = None, attn: Optional[Tensor] = None
                ) -> Tuple[Tensor, Tensor, Optional[Tensor], Optional[Tensor], Tensor, Tensor]:
        attn = x if attn is None else attn
        attn = attn.view(-1, 1) if attn.dim() == 1 else attn
        attn = self.gnn(attn, edge_index)
        return self._pool(x, attn, edge_index, edge_attr, batch)

    def __repr__(self) -> str:
        if self.min_score is None:
            ratio = f'ratio={self.ratio}'
        else:
            ratio = f'min_score={self.min_score}'
        return (f'{self.__class__.__name__}({self.gnn.__class__.__name__}, '
                f'{self.in_channels}, {ratio}, multiplier={self.multiplier})')
