import os
from typing import Callable, Optional, Tuple, Union

import torch
from torch import Tensor
from torch.nn import Parameter, Sigmoid

from ... import _native
from ..._functions import ResGatedAggregateFunction, linear
from ...edge_index import as_edge_index
from ..dense.linear import Linear
from ..inits import zeros
from .gcn_conv import _FLOW_HOOKS
from .message_passing import _FLOATS, _LOW, MessagePassing, _n_dst

# PYGAMD_FUSE_RESGATED=0: ResGatedGraphConv layers start with ``fuse = False`` (read at import)
FUSE_RESGATED = os.environ.get('PYGAMD_FUSE_RESGATED', '1') not in ('', '0')


def _cat_bias(a: Optional[Tensor], b: Optional[Tensor], width: int, like: Tensor):
    """the bias of two stacked transforms of ``width`` outputs each (None: zeros; both None: None)"""
    if a is None and b is None:
        return None
    zero = like.new_zeros(width)
    return torch.cat([zero if a is None else a.float(), zero if b is None else b.float()])


class ResGatedGraphConv(MessagePassing):
    r"""The residual gated graph convolution (GatedGCN) with the constructor arguments, state-dict
    keys (``lin_key.*``, ``lin_query.*``, ``lin_value.*``, ``lin_skip.weight``, ``bias``) and
    forward semantics of ``torch_geometric.nn.ResGatedGraphConv``
    (torch_geometric/nn/conv/res_gated_graph_conv.py:13-148):

    .. math:: x_i' = W_1 x_i + \sum_{j \in N(i)} \sigma(W_3 x_i + W_4 x_j) \odot W_2 x_j

    With ``edge_dim`` the three transforms are ``Linear(in + edge_dim, out)`` on ``cat([x,
    edge_attr])`` per edge.  ``x`` is a tensor or a ``(x_src, x_dst)`` pair.  Routes:

    * fused (device tensors, float32 after widening, ``fuse`` true, ``flow='source_to_target'``,
      the sum aggregation, ``act`` a :class:`torch.nn.Sigmoid` and
      ``_native.resgated_supported(out_channels, edge_dim or 0)``): key, query and value are
      node-level dense transforms — ``[query | value]`` ONE product with stacked weights, the key
      sharing its product with ``lin_skip`` — and ``propagate`` is one kernel forward and two
      backward (``ResGatedAggregateFunction``, csrc/resgated.hip).  With ``edge_dim`` every
      ``Linear`` is split into its node and its edge columns; the kernels rebuild the edge terms
      per slot from the RAW features with the two ``[out, edge_dim]`` matrices ``Wk_e + Wq_e`` and
      ``Wv_e`` in registers.  Nothing of size ``E x out`` is formed or saved;
    * the reference's gather -> ``message`` -> aggregate for everything else (host tensors,
      ``fuse = False``, ``target_to_source``, other aggregations or gates, ``out > 512``,
      ``edge_dim > 32`` or ``out * edge_dim > 2048``) — and whenever the message flow is observed
      or replaced: a propagate, message or aggregate hook, explain mode, or a subclass with its own
      ``message``, ``aggregate``, ``update`` or ``propagate``.

    Half and bfloat16 device inputs are widened to float32 and the result handed back in their
    dtype outside autocast.  ``fuse`` is a per-layer attribute initialised from the environment
    switch ``PYGAMD_FUSE_RESGATED`` (read at import, default ``1``)."""

    def __init__(self, in_channels: Union[int, Tuple[int, int]], out_channels: int,
                 act: Optional[Callable] = Sigmoid(), edge_dim: Optional[int] = None,
                 root_weight: bool = True, bias: bool = True, **kwargs):
        kwargs.setdefault('aggr', 'add')
        super().__init__(**kwargs)
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.act = act
        self.edge_dim = edge_dim
        self.root_weight = root_weight
        if isinstance(in_channels, int):
            in_channels = (in_channels, in_channels)
        edge_dim = edge_dim if edge_dim is not None else 0
        self.lin_key = Linear(in_channels[1] + edge_dim, out_channels)
        self.lin_query = Linear(in_channels[0] + edge_dim, out_channels)
        self.lin_value = Linear(in_channels[0] + edge_dim, out_channels)
        if root_weight:
            self.lin_skip = Linear(in_channels[1], out_channels, bias=False)
        else:
            self.register_parameter('lin_skip', None)
        if bias:
            self.bias = Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.fuse = FUSE_RESGATED
        self.reset_parameters()

    def reset_parameters(self):
        super().reset_parameters()
        self.lin_key.reset_parameters()
        self.lin_query.reset_parameters()
        self.lin_value.reset_parameters()
        if self.lin_skip is not None:
            self.lin_skip.reset_parameters()
        if self.bias is not None:
            zeros(self.bias)

    def _stock_flow(self) -> bool:
        """nobody observes or replaces the message flow (as ``gcn_conv.linear_message_flow``)"""
        kind = type(self)
        for name in ('message', 'aggregate', 'update', 'propagate'):
            if getattr(kind, name) is not getattr(ResGatedGraphConv, name):
                return False
        if getattr(self, 'explain', False):
            return False
        return not any(getattr(self, name, None) for name in _FLOW_HOOKS)

    def _fusable(self, x_src: Tensor, x_dst: Tensor, edge_attr: Optional[Tensor]) -> bool:
        De = self.edge_dim or 0
        if not self._stock_flow():
            return False
        if not (self.fuse and self.flow == 'source_to_target' and self.aggr in ('add', 'sum')
                and isinstance(self.act, Sigmoid) and isinstance(x_dst, Tensor)
                and x_src.is_cuda and x_dst.is_cuda and x_src.dim() == 2 and x_dst.dim() == 2
                and x_src.dtype in _FLOATS and x_dst.dtype in _FLOATS):
            return False
        if De == 0:
            if edge_attr is not None:
                return False
        elif not (isinstance(edge_attr, Tensor) and edge_attr.is_cuda and edge_attr.dim() == 2
                  and edge_attr.size(1) == De and edge_attr.dtype in _FLOATS):
            return False
        return _native.resgated_supported(self.out_channels, De)

    def forward(self, x: Union[Tensor, Tuple[Tensor, Tensor]], edge_index,
                edge_attr: Optional[Tensor] = None) -> Tensor:
        if isinstance(x, Tensor):
            x = (x, x)
        if self._fusable(x[0], x[1], edge_attr):
            return self._forward_fused(x[0], x[1], edge_index, edge_attr)
        # In case edge features are not given, key, query and value are computed in node-level
        # space (res_gated_graph_conv.py:117-124)
        if self.edge_dim is None:
            k = self.lin_key(x[1])
            q = self.lin_query(x[0])
            v = self.lin_value(x[0])
        else:
            k, q, v = x[1], x[0], x[0]
        out = self.propagate(edge_index, k=k, q=q, v=v, edge_attr=edge_attr)
        if self.root_weight:
            out = out + self.lin_skip(x[1])
        if self.bias is not None:
            out = out + self.bias
        return out

    def _forward_fused(self, x_src: Tensor, x_dst: Tensor, edge_index,
                       edge_attr: Optional[Tensor]) -> Tensor:
        F = self.out_channels
        low = x_src.dtype if x_src.dtype in _LOW else None
        xs = x_src.float()
        xd = xs if x_dst is x_src else x_dst.float()
        n_dst = _n_dst(self, x_src, x_dst, edge_index, None)
        graph = as_edge_index(edge_index, xs.size(0), n_dst)
        wk, wq, wv = (lin.weight.float() for lin in (self.lin_key, self.lin_query, self.lin_value))
        ea = w_gate = w_value = None
        if self.edge_dim is not None:
            # Linear(in + De, F) on cat([x, a]) = (node columns) x + (edge columns) a
            n_s, n_d = xs.size(1), xd.size(1)
            w_gate = wk[:, n_d:] + wq[:, n_s:]
            w_value = wv[:, n_s:].contiguous()
            wk, wq, wv = wk[:, :n_d], wq[:, :n_s], wv[:, :n_s]
            ea = edge_attr.float()
        # [query | value]: ONE product with stacked weights, every bias folded in
        qv = linear(xs, torch.cat([wq, wv]),
                    _cat_bias(self.lin_query.bias, self.lin_value.bias, F, xs))
        if self.lin_skip is not None:
            # the key shares its product with lin_skip (both read x_dst), which takes the layer's
            # bias; the key is read in place as the left column block
            ks = linear(xd, torch.cat([wk, self.lin_skip.weight.float()]),
                        _cat_bias(self.lin_key.bias, self.bias, F, xd))
            k, skip = ks[:, :F], ks[:, F:]
        else:
            k = linear(xd, wk, None if self.lin_key.bias is None else self.lin_key.bias.float())
            skip = None if self.bias is None else self.bias.float()
        out = ResGatedAggregateFunction.apply(k, qv, ea, w_gate, w_value, graph, n_dst)
        if skip is not None:
            out = out + skip[:n_dst] if skip.dim() == 2 else out + skip
        if low is not None and not torch.is_autocast_enabled():
            out = out.to(low)
        return out

    def message(self, k_i: Tensor, q_j: Tensor, v_j: Tensor,
                edge_attr: Optional[Tensor]) -> Tensor:
        assert (edge_attr is not None) == (self.edge_dim is not None)
        if edge_attr is not None:
            k_i = self.lin_key(torch.cat([k_i, edge_attr], dim=-1))
            q_j = self.lin_query(torch.cat([q_j, edge_attr], dim=-1))
            v_j = self.lin_value(torch.cat([v_j, edge_attr], dim=-1))
        return self.act(k_i + q_j) * v_j
