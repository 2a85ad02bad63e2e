"""``filter_adj`` and :class:`FilterEdges` (torch_geometric/nn/pool/connect/filter_edges.py).

Routes:

* fused (csrc/pool.hip, ``pygamd_filter_edges``) — an int32 / int64 device ``edge_index`` with
  int64 device node and cluster indices: the node map is built as the reference builds it, then
  three launches (chunk counts, their scan, the write) give the relabelled surviving edges in the
  original order and their ids, where the reference has four ``[E]`` gathers, a mask and three
  boolean-mask compactions with a scan and a host synchronisation each.  One host read: the number
  of kept edges.  ``edge_attr[kept]`` of float32 features goes through ``GatherFunction``, whose
  backward is the scatter-add the gradient needs;
* generic — everything else and ``fuse=False``: the reference's expression."""
from typing import Optional, Tuple

import torch
from torch import Tensor

from .... import _native
from ....utils.num_nodes import maybe_num_nodes
from .._fuse import fuse_default
from ..select import SelectOutput
from .base import Connect, ConnectOutput


def _filter_fusable(edge_index: Tensor, node_index: Tensor, cluster_index: Tensor) -> bool:
    return (edge_index.is_cuda and edge_index.dim() == 2 and edge_index.size(0) == 2
            and edge_index.dtype in (torch.int32, torch.int64)
            and node_index.is_cuda and node_index.dtype == torch.int64
            and cluster_index.is_cuda and cluster_index.dtype == torch.int64)


def _take_edges(edge_attr: Tensor, kept: Tensor) -> Tensor:
    if edge_attr.is_cuda and edge_attr.dtype == torch.float32 and edge_attr.dim() >= 1:
        from ...._functions import GatherFunction
        return GatherFunction.apply(edge_attr, kept, False)
    return edge_attr[kept]


def filter_adj(edge_index: Tensor, edge_attr: Optional[Tensor], node_index: Tensor,
               cluster_index: Optional[Tensor] = None, num_nodes: Optional[int] = None, *,
               fuse: Optional[bool] = None) -> Tuple[Tensor, Optional[Tensor]]:
    r"""Keeps the edges between the nodes ``node_index`` and relabels their endpoints to
    ``cluster_index`` (default: the position in ``node_index``), in the original edge order, with
    the arguments of ``torch_geometric.nn.pool.connect.filter_edges.filter_adj``
    (filter_edges.py:11-36).  ``fuse`` (keyword only; None: ``PYGAMD_FUSE_POOL`` or the measured
    default) allows the edge-filter kernel where it applies."""
    num_nodes = maybe_num_nodes(edge_index, num_nodes)
    if cluster_index is None:
        cluster_index = torch.arange(node_index.size(0), device=node_index.device)
    mask = node_index.new_full((num_nodes, ), -1)
    mask[node_index] = cluster_index
    if fuse is None:
        fuse = fuse_default('filter_adj')
    if fuse and _filter_fusable(edge_index, node_index, cluster_index):
        out, kept = _native.filter_edges(edge_index, mask)
        if edge_attr is not None:
            edge_attr = _take_edges(edge_attr, kept)
        return out, edge_attr
    row, col = edge_index[0], edge_index[1]
    row, col = mask[row.long()], mask[col.long()]
    mask = (row >= 0) & (col >= 0)
    row, col = row[mask], col[mask]
    if edge_attr is not None:
        edge_attr = edge_attr[mask]
    return torch.stack([row, col], dim=0), edge_attr


class FilterEdges(Connect):
    r"""Filters out the edges whose endpoints are not both selected, :math:`\mathbf{A}^{\prime} =
    \mathbf{A}_{\mathbf{i},\mathbf{i}}` (``torch_geometric.nn.pool.connect.FilterEdges``,
    filter_edges.py:39-70); every cluster holds one node.  ``fuse`` routes as :func:`filter_adj`
    does."""

    def __init__(self):
        super().__init__()
        self.fuse = fuse_default('filter_adj')

    def forward(self, select_output: SelectOutput, edge_index: Tensor,
                edge_attr: Optional[Tensor] = None,
                batch: Optional[Tensor] = None) -> ConnectOutput:
        if select_output.num_clusters != select_output.cluster_index.size(0):
            raise ValueError(f"'{self.__class__.__name__}' requires each cluster to contain only "
                             f"one node")
        edge_index, edge_attr = filter_adj(edge_index, edge_attr, select_output.node_index,
                                           select_output.cluster_index,
                                           num_nodes=select_output.num_nodes, fuse=self.fuse)
        batch = self.get_pooled_batch(select_output, batch)
        return ConnectOutput(edge_index, edge_attr, batch)
