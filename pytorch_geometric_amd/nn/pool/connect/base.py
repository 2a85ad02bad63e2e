from dataclasses import dataclass
from typing import Optional

import torch
from torch import Tensor

from ..select import SelectOutput


@dataclass(init=False)
class ConnectOutput:
    r"""The output of a :class:`Connect` module, with the fields and the checks of
    ``torch_geometric.nn.pool.connect.ConnectOutput`` (torch_geometric/nn/pool/connect/base.py:10-48):
    the coarsened graph's ``edge_index`` and its optional ``edge_attr`` and ``batch`` vector."""
    edge_index: Tensor
    edge_attr: Optional[Tensor] = None
    batch: Optional[Tensor] = None

    def __init__(self, edge_index: Tensor, edge_attr: Optional[Tensor] = None,
                 batch: Optional[Tensor] = None):
        if edge_index.dim() != 2:
            raise ValueError(f"Expected 'edge_index' to be two-dimensional "
                             f"(got {edge_index.dim()} dimensions)")
        if edge_index.size(0) != 2:
            raise ValueError(f"Expected 'edge_index' to have size '2' in the first dimension "
                             f"(got '{edge_index.size(0)}')")
        if edge_attr is not None and edge_attr.size(0) != edge_index.size(1):
            raise ValueError(f"Expected 'edge_index' and 'edge_attr' to hold the same number of "
                             f"edges (got {edge_index.size(1)} and {edge_attr.size(0)} edges)")
        self.edge_index = edge_index
        self.edge_attr = edge_attr
        self.batch = batch


class Connect(torch.nn.Module):
    r"""Base class of edge connection operators (``torch_geometric.nn.pool.connect.Connect``):
    decides the edges between the super nodes a :class:`~..select.Select` produced and pools edge
    features and the batch vector."""

    def reset_parameters(self):
        pass

    def forward(self, select_output: SelectOutput, edge_index: Tensor,
                edge_attr: Optional[Tensor] = None,
                batch: Optional[Tensor] = None) -> ConnectOutput:
        raise NotImplementedError

    @staticmethod
    def get_pooled_batch(select_output: SelectOutput,
                         batch: Optional[Tensor]) -> Optional[Tensor]:
        r"""The batch vector of the coarsened graph (connect/base.py:88-106)."""
        if batch is None:
            return batch
        out = torch.arange(select_output.num_clusters, dtype=batch.dtype, device=batch.device)
        return out.scatter_(0, select_output.cluster_index, batch[select_output.node_index])

    def __repr__(self) -> str:
        return f'{self.__class__.__name__}()'
