import copy
import inspect
from typing import Any, Callable, Dict, List, Optional, Union

import torch
from torch import Tensor
from torch.nn import ModuleList

from ...utils import trim_to_layer
from ..conv import GATConv, GATv2Conv, GCNConv, MessagePassing, SAGEConv
from ..conv._act_request import has_forward_hooks, request_activation
from ..norm import normalization_resolver

_ACTS = {'relu': torch.nn.ReLU, 'elu': torch.nn.ELU, 'leaky_relu': torch.nn.LeakyReLU,
         'gelu': torch.nn.GELU, 'tanh': torch.nn.Tanh, 'sigmoid': torch.nn.Sigmoid}


def activation_resolver(act, **kwargs):
    if act is None or callable(act):
        return act
    if isinstance(act, str) and act.lower() in _ACTS:
        return _ACTS[act.lower()](**kwargs)
    raise ValueError(f"Could not resolve activation '{act}'")


class BasicGNN(torch.nn.Module):
    r"""Stack of ``num_layers`` message-passing layers with activation / dropout between them —
    the layer loop of ``torch_geometric.nn.models.BasicGNN``
    (torch_geometric/nn/models/basic_gnn.py:69-274), restricted to ``jk=None``:
    ``in -> hidden -> ... -> hidden -> (out_channels or hidden)``; the last layer has no
    activation; ``num_sampled_*_per_hop`` enables ``trim_to_layer``.

    ``norm`` (a name such as ``'graph_norm'``, ``'layer_norm'``, ``'batch_norm'``, resolved among
    this package's ``nn.norm`` classes with ``norm_kwargs``, or a module) puts a normalisation
    layer behind every layer but the last, in the reference's order: activation first if
    ``act_first``, the norm, the activation otherwise, dropout (basic_gnn.py:258-267).  The copies
    live in ``self.norms`` (an ``Identity`` for the last layer) and ``supports_norm_batch`` says
    whether they take the batch vector.  With a norm the layers are not asked to apply bias + ReLU
    themselves and :class:`GraphSAGE` does not take its fused stack.  With ``norm=None`` there is
    no ``norms`` attribute and nothing differs from a model built before norms were offered.

    ``forward`` takes ``batch`` and ``batch_size`` for those layers as KEYWORD-ONLY arguments.
    The reference has them at positions 5 and 6; this class already had
    ``num_sampled_nodes_per_hop`` and ``num_sampled_edges_per_hop`` there, and positional callers
    keep their meaning."""
    supports_edge_weight: bool = False
    supports_edge_attr: bool = False
    supports_norm_batch: bool = False

    def __init__(self, in_channels: int, hidden_channels: int, num_layers: int,
                 out_channels: Optional[int] = None, dropout: float = 0.0,
                 act: Union[str, Callable, None] = 'relu', act_first: bool = False,
                 act_kwargs=None, norm=None, norm_kwargs: Optional[Dict[str, Any]] = None,
                 jk: Optional[str] = None, **kwargs):
        super().__init__()
        if jk is not None:
            raise NotImplementedError("only jk=None is supported")
        self.in_channels = in_channels
        self.hidden_channels = hidden_channels
        self.num_layers = num_layers
        self.dropout = torch.nn.Dropout(p=dropout)
        self.act = activation_resolver(act, **(act_kwargs or {}))
        self.act_first = act_first
        self.out_channels = out_channels if out_channels is not None else hidden_channels
        self.convs = ModuleList()
        if num_layers > 1:
            self.convs.append(self.init_conv(in_channels, hidden_channels, **kwargs))
            in_channels = hidden_channels
        for _ in range(num_layers - 2):
            self.convs.append(self.init_conv(in_channels, hidden_channels, **kwargs))
            in_channels = hidden_channels
        if out_channels is not None:
            self._is_conv_to_out = True
            self.convs.append(self.init_conv(in_channels, out_channels, **kwargs))
        else:
            self.convs.append(self.init_conv(in_channels, hidden_channels, **kwargs))
        self.norm = norm if isinstance(norm, str) else None
        self.norm_kwargs = norm_kwargs
        if norm is not None:
            layer = normalization_resolver(norm, hidden_channels, **(norm_kwargs or {}))
            if hasattr(layer, 'forward'):
                self.supports_norm_batch = 'batch' in inspect.signature(layer.forward).parameters
            self.norms = ModuleList([copy.deepcopy(layer) for _ in range(num_layers - 1)])
            self.norms.append(torch.nn.Identity())

    def init_conv(self, in_channels: int, out_channels: int, **kwargs) -> MessagePassing:
        raise NotImplementedError

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()
        for norm in getattr(self, 'norms', ()):
            if hasattr(norm, 'reset_parameters'):
                norm.reset_parameters()

    def forward(self, x: Tensor, edge_index, edge_weight: Optional[Tensor] = None,
                edge_attr: Optional[Tensor] = None,
                num_sampled_nodes_per_hop: Optional[List[int]] = None,
                num_sampled_edges_per_hop: Optional[List[int]] = None, *,
                batch: Optional[Tensor] = None, batch_size: Optional[int] = None) -> Tensor:
        norms = getattr(self, 'norms', None)
        if (num_sampled_nodes_per_hop is not None and isinstance(edge_weight, Tensor)
                and isinstance(edge_attr, Tensor)):
            raise NotImplementedError("'trim_to_layer' functionality does not yet support "
                                      "trimming of both 'edge_weight' and 'edge_attr'")
        # ReLU stacks of layers that end in `out + bias` (GCNConv, GATConv, RGCNConv): the layer
        # applies bias + ReLU itself in one pass (_functions.BiasActFunction) instead of an ATen
        # add here and an ATen clamp there (and two more passes in the backward).  The request is
        # per CALL (a thread-local slot naming the conv object, consumed by that layer call:
        # nn/conv/_act_request.py), never module state; a layer with forward hooks is not asked
        # (its hooks must see the reference's pre-activation output).
        fuse_ok = isinstance(self.act, torch.nn.ReLU) and isinstance(x, Tensor) and x.is_cuda \
            and x.dtype == torch.float32 and not has_forward_hooks(self.act) and norms is None
        for i, conv in enumerate(self.convs):
            if num_sampled_nodes_per_hop is not None:
                x, edge_index, value = trim_to_layer(
                    i, num_sampled_nodes_per_hop, num_sampled_edges_per_hop, x, edge_index,
                    edge_weight if edge_weight is not None else edge_attr)
                if edge_weight is not None:
                    edge_weight = value
                else:
                    edge_attr = value
            fused = fuse_ok and i < self.num_layers - 1 and hasattr(conv, 'bias') \
                and type(conv).__name__ in ('GCNConv', 'GATConv', 'GATv2Conv', 'RGCNConv',
                                            'FastRGCNConv') \
                and type(conv).__module__.startswith('pytorch_geometric_amd') \
                and not has_forward_hooks(conv)
            with request_activation(conv, 'relu' if fused else None):
                if self.supports_edge_weight and self.supports_edge_attr:
                    x = conv(x, edge_index, edge_weight=edge_weight, edge_attr=edge_attr)
                elif self.supports_edge_weight:
                    x = conv(x, edge_index, edge_weight=edge_weight)
                elif self.supports_edge_attr:
                    x = conv(x, edge_index, edge_attr=edge_attr)
                else:
                    x = conv(x, edge_index)
            if i < self.num_layers - 1:
                if norms is not None:
                    if self.act is not None and self.act_first:
                        x = self.act(x)
                    x = norms[i](x, batch, batch_size) if self.supports_norm_batch \
                        else norms[i](x)
                    if self.act is not None and not self.act_first:
                        x = self.act(x)
                elif self.act is not None and not fused:
                    x = self.act(x)
                x = self.dropout(x)
        return x

    def __repr__(self) -> str:
        return (f'{self.__class__.__name__}({self.in_channels}, '
                f'{self.out_channels}, num_layers={self.num_layers})')


class GCN(BasicGNN):
    """:class:`GCNConv` stack (basic_gnn.py:389-432)."""
    supports_edge_weight = True

    def init_conv(self, in_channels: int, out_channels: int, **kwargs) -> MessagePassing:
        return GCNConv(in_channels, out_channels, **kwargs)


class GraphSAGE(BasicGNN):
    """:class:`SAGEConv` stack (basic_gnn.py:434-476).  With plain mean/sum layers, ReLU and no
    dropout the whole stack runs through :mod:`._fused_sage` (set ``fuse_stack = False`` to force
    the layer-by-layer path)."""
    fuse_stack: bool = True

    def init_conv(self, in_channels, out_channels: int, **kwargs) -> MessagePassing:
        return SAGEConv(in_channels, out_channels, **kwargs)

    def forward(self, x: Tensor, edge_index, edge_weight: Optional[Tensor] = None,
                edge_attr: Optional[Tensor] = None,
                num_sampled_nodes_per_hop: Optional[List[int]] = None,
                num_sampled_edges_per_hop: Optional[List[int]] = None, *,
                batch: Optional[Tensor] = None, batch_size: Optional[int] = None) -> Tensor:
        from . import _fused_sage, _fused_sage_hops
        if getattr(self, 'norms', None) is not None:  # the fused stack has no place for a norm
            return super().forward(x, edge_index, edge_weight, edge_attr,
                                   num_sampled_nodes_per_hop, num_sampled_edges_per_hop,
                                   batch=batch, batch_size=batch_size)
        if _fused_sage_hops.eligible(self, x, edge_index, num_sampled_nodes_per_hop,
                                     num_sampled_edges_per_hop):
            return _fused_sage_hops.run(self, x, edge_index, num_sampled_nodes_per_hop,
                                        num_sampled_edges_per_hop)
        if _fused_sage.eligible(self, x, edge_index, num_sampled_nodes_per_hop is not None):
            return _fused_sage.run(self, x, edge_index)
        return super().forward(x, edge_index, edge_weight, edge_attr,
                               num_sampled_nodes_per_hop, num_sampled_edges_per_hop)


class GAT(BasicGNN):
    """:class:`GATConv` stack (basic_gnn.py:528-597): hidden layers concatenate ``heads`` of
    width ``hidden // heads``; an explicit output layer averages its heads.  ``v2=True`` builds
    :class:`GATv2Conv` layers instead."""
    supports_edge_attr = True

    def init_conv(self, in_channels, out_channels: int, **kwargs) -> MessagePassing:
        v2 = kwargs.pop('v2', False)
        heads = kwargs.pop('heads', 1)
        concat = kwargs.pop('concat', True)
        # do not use concatenation in the last layer when out_channels was given explicitly
        if getattr(self, '_is_conv_to_out', False):
            concat = False
        if concat and out_channels % heads != 0:
            raise ValueError(f"Ensure that the number of output channels of 'GATConv' (got "
                             f"'{out_channels}') is divisible by the number of heads "
                             f"(got '{heads}')")
        if concat:
            out_channels = out_channels // heads
        Conv = GATv2Conv if v2 else GATConv
        return Conv(in_channels, out_channels, heads=heads, concat=concat,
                    dropout=self.dropout.p, **kwargs)
