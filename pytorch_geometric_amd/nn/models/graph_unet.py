"""``GraphUNet`` (torch_geometric/nn/models/graph_unet.py:17-153): the reference's arguments,
parameter names (state dicts interchange), ``__repr__`` and ``augment_adj``; the squared adjacency
of ``augment_adj`` comes from the sparse-sparse product kernels of csrc/spgemm.hip."""
from typing import Callable, List, Optional, Tuple, Union

import torch
from torch import Tensor

from ... import _spgemm
from ...utils import add_self_loops, remove_self_loops
from ..conv import GCNConv
from ..pool import TopKPooling


def _act(act: Union[str, Callable, None]) -> Callable:
    if callable(act):
        return act
    fn = getattr(torch.nn.functional, str(act).lower(), None)
    if fn is None:
        raise ValueError(f"Could not resolve '{act}' among torch.nn.functional")
    return fn


class GraphUNet(torch.nn.Module):
    r"""The Graph U-Net of `"Graph U-Nets" <https://arxiv.org/abs/1905.05178>`_: ``depth`` rounds
    of (square the adjacency, ``TopKPooling``, ``GCNConv(improved=True)``) and the way back up
    through the kept nodes.  ``fuse`` (a per-module attribute; initial value from
    ``PYGAMD_FUSE_SPGEMM`` or the measured default) sends ``augment_adj`` to the kernels."""

    def __init__(self, in_channels: int, hidden_channels: int, out_channels: int, depth: int,
                 pool_ratios: Union[float, List[float]] = 0.5, sum_res: bool = True,
                 act: Union[str, Callable] = 'relu'):
        super().__init__()
        assert depth >= 1
        self.in_channels = in_channels
        self.hidden_channels = hidden_channels
        self.out_channels = out_channels
        self.depth = depth
        if not isinstance(pool_ratios, (list, tuple)):
            pool_ratios = [pool_ratios] * depth
        pool_ratios = list(pool_ratios)[:depth]
        self.pool_ratios = pool_ratios + [pool_ratios[-1]] * (depth - len(pool_ratios))
        self.act = _act(act)
        self.sum_res = sum_res
        self.fuse = _spgemm.fuse_default()

        channels = hidden_channels
        self.down_convs = torch.nn.ModuleList()
        self.pools = torch.nn.ModuleList()
        self.down_convs.append(GCNConv(in_channels, channels, improved=True))
        for i in range(depth):
            self.pools.append(TopKPooling(channels, self.pool_ratios[i]))
            self.down_convs.append(GCNConv(channels, channels, improved=True))
        in_channels = channels if sum_res else 2 * channels
        self.up_convs = torch.nn.ModuleList()
        for _ in range(depth - 1):
            self.up_convs.append(GCNConv(in_channels, channels, improved=True))
        self.up_convs.append(GCNConv(in_channels, out_channels, improved=True))
        self.reset_parameters()

    def reset_parameters(self):
        for conv in self.down_convs:
            conv.reset_parameters()
        for pool in self.pools:
            pool.reset_parameters()
        for conv in self.up_convs:
            conv.reset_parameters()

    def forward(self, x: Tensor, edge_index: Tensor, batch: Optional[Tensor] = None,
                edge_weight: Optional[Tensor] = None) -> Tensor:
        if batch is None:
            batch = edge_index.new_zeros(x.size(0))
        if edge_weight is None:
            edge_weight = x.new_ones(edge_index.size(1))
        assert edge_weight.dim() == 1
        assert edge_weight.size(0) == edge_index.size(1)

        x = self.act(self.down_convs[0](x, edge_index, edge_weight))
        xs, edge_indices, edge_weights, perms = [x], [edge_index], [edge_weight], []
        for i in range(1, self.depth + 1):
            edge_index, edge_weight = self.augment_adj(edge_index, edge_weight, x.size(0))
            x, edge_index, edge_weight, batch, perm, _ = self.pools[i - 1](
                x, edge_index, edge_weight, batch)
            x = self.act(self.down_convs[i](x, edge_index, edge_weight))
            if i < self.depth:
                xs += [x]
                edge_indices += [edge_index]
                edge_weights += [edge_weight]
            perms += [perm]

        for i in range(self.depth):
            j = self.depth - 1 - i
            res, perm = xs[j], perms[j]
            up = torch.zeros_like(res)
            up[perm] = x
            x = res + up if self.sum_res else torch.cat((res, up), dim=-1)
            x = self.up_convs[i](x, edge_indices[j], edge_weights[j])
            x = self.act(x) if i < self.depth - 1 else x
        return x

    def augment_adj(self, edge_index: Tensor, edge_weight: Tensor,
                    num_nodes: int) -> Tuple[Tensor, Tensor]:
        """``(A + I)^2`` without its diagonal (graph_unet.py:138-148): remove self loops, add self
        loops, coalesce, the product, remove self loops.  The edges come back row-major with
        ascending columns, the order the reference's CSR -> COO gives."""
        edge_index, edge_weight = remove_self_loops(edge_index, edge_weight)
        edge_index, edge_weight = add_self_loops(edge_index, edge_weight, num_nodes=num_nodes)
        n = int(num_nodes)
        out = None
        if self.fuse and _spgemm.eligible(edge_index, n, edge_weight):
            from ... import _native
            from ...utils import coalesce
            # the coalesced list is row-major with unique columns: both operands as they are
            (row, col), weight = coalesce((edge_index[0], edge_index[1]), edge_weight, num_nodes=n)
            ptr = _native.index2ptr(row.contiguous(), n)
            try:
                out = _native.spgemm(ptr, col, weight, ptr, col, weight, n, n, n)
            except _native.SpgemmUnsupported:   # the long tier's envelope
                out = None
        if out is None:
            row, col = edge_index[0], edge_index[1]
            out = _spgemm.generic(row, col, edge_weight, row, col, edge_weight, n, n, n)
        rowptr, col, weight = out
        row = _spgemm.ptr2index(rowptr, col.numel())
        return remove_self_loops(torch.stack([row, col]), weight)

    def __repr__(self) -> str:
        return (f'{self.__class__.__name__}({self.in_channels}, {self.hidden_channels}, '
                f'{self.out_channels}, depth={self.depth}, pool_ratios={self.pool_ratios})')
