import os
from typing import Callable, Optional, Tuple, Union

import torch
from torch import Tensor

from ... import _native
from ..._functions import GineAggregateFunction, SpmmFunction
from ...edge_index import as_edge_index
from ..dense.linear import Linear
from ..inits import reset
from .message_passing import _LOW, MessagePassing, _n_dst, _pair

# PYGAMD_FUSE_GINE=0: GINEConv layers start with ``fuse = False`` (read at import)
FUSE_GINE = os.environ.get('PYGAMD_FUSE_GINE', '1') not in ('', '0')


class GINConv(MessagePassing):
    r"""Graph isomorphism operator with the constructor arguments, state-dict keys (``eps``,
    ``nn.*``) and forward semantics of ``torch_geometric.nn.GINConv``
    (torch_geometric/nn/conv/gin_conv.py:19-101):

    .. math:: x_i' = h_\Theta\big((1 + \epsilon) x_i + \sum_{j \in N(i)} x_j\big)

    ``eps`` is a parameter with ``train_eps`` and a buffer otherwise.  ``x`` is a tensor,
    ``(x_src, x_dst)`` or ``(x_src, None)`` (no self term).  Routes: float32 device tensors with
    ``flow='source_to_target'`` and the sum aggregation take the CSR sum SpMM
    (``SpmmFunction``); everything else takes the generic ``propagate``."""

    def __init__(self, nn: Callable, eps: float = 0., train_eps: bool = False, **kwargs):
        kwargs.setdefault('aggr', 'add')
        super().__init__(**kwargs)
        self.nn = nn
        self.initial_eps = eps
        if train_eps:
            self.eps = torch.nn.Parameter(torch.empty(1))
        else:
            self.register_buffer('eps', torch.empty(1))
        self.fuse = True
        self.reset_parameters()

    def reset_parameters(self):
        super().reset_parameters()
        reset(self.nn)
        self.eps.data.fill_(self.initial_eps)

    def forward(self, x: Union[Tensor, Tuple[Tensor, Optional[Tensor]]], edge_index,
                size=None) -> Tensor:
        x_src, x_dst = _pair(x)
        if (x_src.is_cuda and x_src.dtype == torch.float32 and self.fuse
                and self.flow == 'source_to_target' and self.aggr in ('add', 'sum')
                and x_src.dim() == 2):
            n_dst = _n_dst(self, x_src, x_dst, edge_index, size)
            graph = as_edge_index(edge_index, x_src.size(0), n_dst)
            out = SpmmFunction.apply(x_src, None, graph, 'sum', 'coo')
        else:
            out = self.propagate(edge_index, x=(x_src, x_dst), size=size)
        if x_dst is not None:
            out = out + (1 + self.eps) * x_dst[:out.size(0)]
        return self.nn(out)

    def message(self, x_j: Tensor) -> Tensor:
        return x_j

    def __repr__(self) -> str:
        return f'{type(self).__name__}(nn={self.nn})'


class GINEConv(MessagePassing):
    r"""The edge-feature variant of :class:`GINConv`, with the constructor arguments, state-dict
    keys (``eps``, ``nn.*``, with ``edge_dim`` also ``lin.weight`` and ``lin.bias``) and forward
    semantics of ``torch_geometric.nn.GINEConv`` (torch_geometric/nn/conv/gin_conv.py:104-207):

    .. math:: x_i' = h_\Theta\big((1 + \epsilon) x_i + \sum_{j \in N(i)}
              \mathrm{ReLU}(x_j + e_{ji})\big)

    where ``e`` is ``edge_attr`` itself (``edge_dim=None``: it must have the width of ``x``) or
    ``lin(edge_attr)``.  Routes:

    * fused (device tensors, float32 after widening, ``fuse`` true, ``flow='source_to_target'``,
      the sum aggregation and ``_native.gine_supported(F, edge_dim or 0)``): ONE kernel per
      direction (``GineAggregateFunction``, csrc/gine.hip).  The ReLU sits between the edge term
      and the sum, so the message is rebuilt per slot in registers: with ``edge_dim`` every lane
      keeps its columns' rows of ``lin.weight`` and reads the RAW ``edge_dim`` features of a
      slot, and nothing of size ``E x F`` is formed or saved;
    * generic gather -> ``message`` -> scatter for everything else (host tensors, ``fuse =
      False``, ``target_to_source``, other aggregations, ``F > 512``, ``edge_dim > 32`` or
      ``F * edge_dim > 4096``).

    Half and bfloat16 device inputs are widened to float32 and the aggregate handed back in
    their dtype outside autocast.  ``fuse`` is a per-layer attribute initialised from the
    environment switch ``PYGAMD_FUSE_GINE`` (read at import, default ``1``)."""

    def __init__(self, nn: torch.nn.Module, eps: float = 0., train_eps: bool = False,
                 edge_dim: Optional[int] = None, **kwargs):
        kwargs.setdefault('aggr', 'add')
        super().__init__(**kwargs)
        self.nn = nn
        self.initial_eps = eps
        if train_eps:
            self.eps = torch.nn.Parameter(torch.empty(1))
        else:
            self.register_buffer('eps', torch.empty(1))
        self.lin = None
        if edge_dim is not None:
            first = self.nn[0] if isinstance(self.nn, torch.nn.Sequential) else self.nn
            if hasattr(first, 'in_features'):
                in_channels = first.in_features
            elif hasattr(first, 'in_channels'):
                in_channels = first.in_channels
            else:
                raise ValueError("Could not infer input channels from `nn`.")
            self.lin = Linear(edge_dim, in_channels)
        self.edge_dim = edge_dim
        self.fuse = FUSE_GINE
        self.reset_parameters()

    def reset_parameters(self):
        reset(self.nn)
        self.eps.data.fill_(self.initial_eps)
        if self.lin is not None:
            self.lin.reset_parameters()

    def _check_width(self, x_src: Tensor, edge_attr: Tensor):
        if self.lin is None and x_src.size(-1) != edge_attr.size(-1):
            raise ValueError("Node and edge feature dimensionalities do not match. Consider "
                             "setting the 'edge_dim' attribute of 'GINEConv'")

    def forward(self, x: Union[Tensor, Tuple[Tensor, Optional[Tensor]]], edge_index,
                edge_attr: Optional[Tensor] = None, size=None) -> Tensor:
        x_src, x_dst = _pair(x)
        if isinstance(edge_attr, Tensor):
            self._check_width(x_src, edge_attr)
        F = x_src.size(-1)
        De = 0 if self.lin is None else self.edge_dim
        fused = (x_src.is_cuda and isinstance(edge_attr, Tensor) and edge_attr.is_cuda
                 and x_src.dim() == 2 and edge_attr.dim() == 2
                 and x_src.dtype in (torch.float32,) + _LOW
                 and edge_attr.dtype in (torch.float32,) + _LOW
                 and self.fuse and self.flow == 'source_to_target'
                 and self.aggr in ('add', 'sum') and edge_attr.size(1) == (De or F)
                 and _native.gine_supported(F, De))
        if fused:
            low = x_src.dtype if x_src.dtype in _LOW else None
            n_dst = _n_dst(self, x_src, x_dst, edge_index, size)
            graph = as_edge_index(edge_index, x_src.size(0), n_dst)
            weight = bias = None
            if self.lin is not None:
                weight = self.lin.weight.float()
                bias = None if self.lin.bias is None else self.lin.bias.float()
            xs = x_src.float()
            xr = None if x_dst is None else (xs if x_dst is x_src else x_dst.float())
            out = GineAggregateFunction.apply(xs, xr, None if xr is None else self.eps.float(),
                                              edge_attr.float(), weight, bias, graph, n_dst)
            if low is not None and not torch.is_autocast_enabled():
                out = out.to(low)
            return self.nn(out)
        out = self.propagate(edge_index, x=(x_src, x_dst), edge_attr=edge_attr, size=size)
        if x_dst is not None:
            out = out + (1 + self.eps) * x_dst[:out.size(0)]
        return self.nn(out)

    def message(self, x_j: Tensor, edge_attr: Tensor) -> Tensor:
        self._check_width(x_j, edge_attr)
        if self.lin is not None:
            edge_attr = self.lin(edge_attr)
        return (x_j + edge_attr).relu()

    def __repr__(self) -> str:
        return f'{type(self).__name__}(nn={self.nn})'
