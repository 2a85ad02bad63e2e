from dataclasses import dataclass
from typing import Optional

import torch
from torch import Tensor


@dataclass(init=False)
class SelectOutput:
    r"""The output of a :class:`Select` module, with the fields and the checks of
    ``torch_geometric.nn.pool.select.SelectOutput`` (torch_geometric/nn/pool/select/base.py:8-62):
    an assignment of the selected nodes ``node_index`` to the clusters ``cluster_index``, out of
    ``num_nodes`` nodes into ``num_clusters`` clusters, with an optional ``weight`` per
    assignment."""
    node_index: Tensor
    num_nodes: int
    cluster_index: Tensor
    num_clusters: int
    weight: Optional[Tensor] = None

    def __init__(self, node_index: Tensor, num_nodes: int, cluster_index: Tensor,
                 num_clusters: int, weight: Optional[Tensor] = None):
        if node_index.dim() != 1:
            raise ValueError(f"Expected 'node_index' to be one-dimensional "
                             f"(got {node_index.dim()} dimensions)")
        if cluster_index.dim() != 1:
            raise ValueError(f"Expected 'cluster_index' to be one-dimensional "
                             f"(got {cluster_index.dim()} dimensions)")
        if node_index.numel() != cluster_index.numel():
            raise ValueError(f"Expected 'node_index' and 'cluster_index' to hold the same number "
                             f"of values (got {node_index.numel()} and {cluster_index.numel()} "
                             f"values)")
        if weight is not None and weight.dim() != 1:
            raise ValueError(f"Expected 'weight' vector to be one-dimensional "
                             f"(got {weight.dim()} dimensions)")
        if weight is not None and weight.numel() != node_index.numel():
            raise ValueError(f"Expected 'weight' to hold {node_index.numel()} values "
                             f"(got {weight.numel()} values)")
        self.node_index = node_index
        self.num_nodes = num_nodes
        self.cluster_index = cluster_index
        self.num_clusters = num_clusters
        self.weight = weight


class Select(torch.nn.Module):
    r"""Base class of node selections (``torch_geometric.nn.pool.select.Select``): maps the nodes
    of a graph to the super nodes of the coarsened one and returns a :class:`SelectOutput`."""

    def reset_parameters(self):
        pass

    def forward(self, *args, **kwargs) -> SelectOutput:
        raise NotImplementedError

    def __repr__(self) -> str:
        return f'{self.__class__.__name__}()'
