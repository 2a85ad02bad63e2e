"""Graph-level readouts: ``global_add_pool``, ``global_mean_pool`` and ``global_max_pool`` with the
arguments of ``torch_geometric.nn.pool`` (torch_geometric/nn/pool/glob.py:9-106).  Each is one
``scatter`` over the batch vector; ``batch=None`` reduces all nodes into one graph.  The node
dimension is ``-2``, or ``-1`` for a one-dimensional ``x``.  Float32 device tensors go through this
package's ``scatter``; host tensors and other dtypes through the same reduction in plain torch.

The geometric searches ``fps``, ``knn``, ``knn_graph``, ``radius``, ``radius_graph`` and ``nearest``
live in :mod:`.cluster`; the hierarchical pooling layers ``TopKPooling`` and ``SAGPooling`` in
:mod:`.topk_pool` and :mod:`.sag_pool`, over ``topk`` / ``SelectTopK`` (:mod:`.select`) and
``filter_adj`` / ``FilterEdges`` (:mod:`.connect`)."""
from typing import Optional

import torch
from torch import Tensor

from ...utils import scatter
from .cluster import fps, knn, knn_graph, nearest, radius, radius_graph
from .connect import FilterEdges, filter_adj
from .sag_pool import SAGPooling
from .select import SelectTopK, topk
from .topk_pool import TopKPooling


def _node_dim(x: Tensor) -> int:
    return -1 if isinstance(x, Tensor) and x.dim() == 1 else -2


def _scatter(x: Tensor, batch: Tensor, dim: int, size: Optional[int], reduce: str) -> Tensor:
    if x.is_cuda and batch.is_cuda and x.dtype == torch.float32:
        return scatter(x, batch, dim=dim, dim_size=size, reduce=reduce)
    dim = x.dim() + dim
    if size is None:
        size = int(batch.max()) + 1 if batch.numel() > 0 else 0
    shape = list(x.shape)
    shape[dim] = size
    index = batch.long().view([-1 if d == dim else 1 for d in range(x.dim())]).expand_as(x)
    how = {'sum': 'sum', 'mean': 'mean', 'max': 'amax'}[reduce]
    return x.new_zeros(shape).scatter_reduce(dim, index, x, how, include_self=False)


def global_add_pool(x: Tensor, batch: Optional[Tensor], size: Optional[int] = None) -> Tensor:
    r"""Sums the node features of each graph: :math:`\mathbf{r}_i = \sum_{n=1}^{N_i}
    \mathbf{x}_n`."""
    dim = _node_dim(x)
    if batch is None:
        return x.sum(dim=dim, keepdim=x.dim() <= 2)
    return _scatter(x, batch, dim, size, 'sum')


def global_mean_pool(x: Tensor, batch: Optional[Tensor], size: Optional[int] = None) -> Tensor:
    r"""Averages the node features of each graph: :math:`\mathbf{r}_i = \frac{1}{N_i}
    \sum_{n=1}^{N_i} \mathbf{x}_n`."""
    dim = _node_dim(x)
    if batch is None:
        return x.mean(dim=dim, keepdim=x.dim() <= 2)
    return _scatter(x, batch, dim, size, 'mean')


def global_max_pool(x: Tensor, batch: Optional[Tensor], size: Optional[int] = None) -> Tensor:
    r"""The channel-wise maximum over the nodes of each graph: :math:`\mathbf{r}_i =
    \mathrm{max}_{n=1}^{N_i} \mathbf{x}_n`."""
    dim = _node_dim(x)
    if batch is None:
        return x.max(dim=dim, keepdim=x.dim() <= 2)[0]
    return _scatter(x, batch, dim, size, 'max')


__all__ = ['global_add_pool', 'global_mean_pool', 'global_max_pool',
           'fps', 'knn', 'knn_graph', 'radius', 'radius_graph', 'nearest',
           'TopKPooling', 'SAGPooling', 'SelectTopK', 'FilterEdges', 'topk', 'filter_adj']
