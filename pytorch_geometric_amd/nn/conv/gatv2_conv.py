import weakref
from typing import Optional, Tuple, Union

import torch
import torch.nn.functional as F
from torch import Tensor
from torch.nn import Parameter

from ... import _native
from ..._functions import Gatv2AttendFunction, Gatv2ScoreFunction, SpmmFunction, bias_act
from ...edge_index import EdgeIndex, as_edge_index
from ...utils import add_self_loops, remove_self_loops
from .._host import softmax
from ..dense.linear import Linear
from ..inits import glorot, zeros
from ._act_request import requested_activation
from .message_passing import MessagePassing


# self-looped edge lists of raw `edge_index` tensors: id -> (weakref, version, num_nodes, tensor)
_LOOPS = {}


class GATv2Conv(MessagePassing):
    r"""GATv2 operator with the constructor arguments, parameter names (``lin_l``, ``lin_r``,
    ``att``, optional ``lin_edge`` / ``res``, ``bias``) and forward semantics of
    ``torch_geometric.nn.GATv2Conv`` (torch_geometric/nn/conv/gatv2_conv.py:27-382):

    .. math:: \alpha_{ij} = \mathrm{softmax}_j\, a^\top \mathrm{LeakyReLU}(W_l x_j + W_r x_i),
              \qquad x_i' = \big\Vert_h \sum_j \alpha^h_{ij} W_l^h x_j \;(\text{or the head mean}).

    The non-linearity sits inside the dot product, so every edge needs the whole source row.  Routes:

    * fused (float32 device tensors, no edge features, nothing between score and aggregation
      observable): ONE kernel per destination row gathers each ``x_l[j]`` once for the score, an
      online softmax and the weighted sum (``Gatv2AttendFunction``);
    * score mode (dropout on the coefficients in training, ``return_attention_weights``): the same
      kernel writes ``alpha [E, H]`` only, the multi-head weighted SpMM aggregates;
    * generic gather -> ``edge_update`` -> scatter for ``edge_dim``, host tensors, ``fuse =
      False``, ``target_to_source`` and head layouts the kernels do not serve (``H * C > 512``).
    """

    def __init__(self, in_channels: Union[int, Tuple[int, int]], out_channels: int,
                 heads: int = 1, concat: bool = True, negative_slope: float = 0.2,
                 dropout: float = 0.0, add_self_loops: bool = True,
                 edge_dim: Optional[int] = None, fill_value: Union[float, Tensor, str] = 'mean',
                 bias: bool = True, share_weights: bool = False, residual: bool = False,
                 **kwargs):
        kwargs.setdefault('aggr', 'add')
        super().__init__(node_dim=0, **kwargs)
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.concat, self.negative_slope, self.dropout = concat, negative_slope, dropout
        self.add_self_loops, self.edge_dim = add_self_loops, edge_dim
        self.fill_value, self.residual, self.share_weights = fill_value, residual, share_weights
        width = heads * out_channels
        in_l, in_r = (in_channels, in_channels) if isinstance(in_channels, int) else in_channels
        self.lin_l = Linear(in_l, width, bias=bias, weight_initializer='glorot')
        self.lin_r = self.lin_l if share_weights else Linear(in_r, width, bias=bias,
                                                             weight_initializer='glorot')
        self.att = Parameter(torch.empty(1, heads, out_channels))
        self.lin_edge = None if edge_dim is None else Linear(edge_dim, width, bias=False,
                                                             weight_initializer='glorot')
        out_width = width if concat else out_channels
        if residual:
            self.res = Linear(in_r, out_width, bias=False, weight_initializer='glorot')
        else:
            self.register_parameter('res', None)
        self.register_parameter('bias', Parameter(torch.empty(out_width)) if bias else None)
        self.fuse = True
        self.reset_parameters()

    def reset_parameters(self):
        super().reset_parameters()
        self.lin_l.reset_parameters()
        self.lin_r.reset_parameters()
        if self.lin_edge is not None:
            self.lin_edge.reset_parameters()
        if self.res is not None:
            self.res.reset_parameters()
        glorot(self.att)
        zeros(self.bias)

    def _rewrite_loops(self, edge_index: Tensor, edge_attr: Optional[Tensor], num_nodes: int):
        """remove_self_loops + add_self_loops (gatv2_conv.py:313-317).  Host edge attributes with a
        reduction as ``fill_value`` get their loop attributes from plain torch."""
        ei, ea = remove_self_loops(edge_index, edge_attr)
        fill = self.fill_value
        if ea is not None and isinstance(fill, str) and not ea.is_cuda:
            how = {'add': 'sum', 'sum': 'sum', 'mean': 'mean', 'min': 'amin', 'max': 'amax',
                   'mul': 'prod'}[fill]
            rows = ea.view(ea.size(0), -1)
            where = ei[1].long().view(-1, 1).expand_as(rows)
            fill = rows.new_zeros(num_nodes, rows.size(1)).scatter_reduce(
                0, where, rows, how, include_self=False).view(num_nodes, *ea.shape[1:])
        return add_self_loops(ei, ea, fill_value=fill, num_nodes=num_nodes)

    def _with_self_loops(self, edge_index: Tensor, edge_attr: Optional[Tensor], num_nodes: int):
        """Drop existing self-loops, then add one per node.  Without edge features the augmented
        edge list is cached per input tensor and shared by every GATv2Conv layer (the result does
        not depend on the layer), so a stack of layers sorts ONE derived graph."""
        if edge_attr is not None:
            return self._rewrite_loops(edge_index, edge_attr, num_nodes)
        key = id(edge_index)
        hit = _LOOPS.get(key)
        if hit is not None:
            ref, version, n, cached = hit
            if ref() is edge_index and version == edge_index._version and n == num_nodes:
                return cached, None
        ei, _ = self._rewrite_loops(edge_index, None, num_nodes)
        if len(_LOOPS) >= 4:
            _LOOPS.pop(next(iter(_LOOPS)))
        _LOOPS[key] = (weakref.ref(edge_index, lambda _, key=key: _LOOPS.pop(key, None)),
                       edge_index._version, num_nodes, ei)
        return ei, None

    def forward(self, x: Union[Tensor, Tuple[Tensor, Optional[Tensor]]], edge_index,
                edge_attr: Optional[Tensor] = None,
                return_attention_weights: Optional[bool] = None):
        H, C = self.heads, self.out_channels
        res = None
        if isinstance(x, Tensor):
            assert x.dim() == 2
            if self.res is not None:
                res = self.res(x)
            x_l = self.lin_l(x).view(-1, H, C)
            x_r = x_l if self.share_weights else self.lin_r(x).view(-1, H, C)
        else:
            x_l, x_r = x[0], x[1]
            assert x[0].dim() == 2
            if x_r is not None and self.res is not None:
                res = self.res(x_r)
            x_l = self.lin_l(x_l).view(-1, H, C)
            if x_r is not None:
                x_r = self.lin_r(x_r).view(-1, H, C)
        assert x_l is not None and x_r is not None
        # the kernels compute in float32: half / bf16 projections are widened here and the result
        # handed back in their dtype outside autocast (as GATConv does)
        low = None
        if x_l.is_cuda and x_l.dtype in (torch.float16, torch.bfloat16):
            low = x_l.dtype
            same = x_r is x_l
            x_l = x_l.float()
            x_r = x_l if same else x_r.float()
            res = None if res is None else res.float()
        att = self.att if self.att.dtype == x_l.dtype else self.att.to(x_l.dtype)

        if self.add_self_loops and isinstance(edge_index, EdgeIndex):
            # handles get the same remove + add self-loops treatment as tensors; the result is
            # cached on the handle
            handle = edge_index
            n = min(handle.sparse_size)
            given = edge_attr

            def build():
                ei, ea = self._rewrite_loops(handle.edge_index, given, n)
                out = EdgeIndex(ei, handle.sparse_size, validate=False)
                out.atomic_backward = handle.atomic_backward
                return out, ea

            if edge_attr is None:
                edge_index, edge_attr = handle.derived(('self_loops', n), build)
            else:
                edge_index, edge_attr = build()
        elif self.add_self_loops and isinstance(edge_index, Tensor):
            n = min(x_l.size(0), x_r.size(0))
            edge_index, edge_attr = self._with_self_loops(edge_index, edge_attr, n)

        want_alpha = bool(return_attention_weights)
        native = (x_l.is_cuda and x_l.dtype == torch.float32 and x_r.dtype == torch.float32
                  and self.fuse and edge_attr is None and self.flow == 'source_to_target'
                  and _native.gatv2_supported(H, C))
        alpha = None
        if native:
            n_src, n_dst = x_l.size(0), x_r.size(0)
            graph = as_edge_index(edge_index, n_src, n_dst)
            if want_alpha or (self.training and self.dropout > 0):
                # the coefficients are observable (dropout acts on them, or the caller asked):
                # score kernel -> dropout -> multi-head weighted SpMM
                alpha_slot = Gatv2ScoreFunction.apply(x_l, x_r, att, graph, self.negative_slope,
                                                      n_dst)
                weights = F.dropout(alpha_slot, p=self.dropout, training=self.training)
                out = SpmmFunction.apply(x_l.reshape(n_src, H * C), weights, graph, 'sum', 'slot')
                out = out.view(-1, H, C)
                if want_alpha:
                    # the POST-dropout coefficients (what edge_update returns in the reference,
                    # gatv2_conv.py:373-375), back in the caller's edge order
                    alpha = torch.empty_like(weights)
                    alpha[graph.by_dst().perm.long()] = weights
            else:
                out = Gatv2AttendFunction.apply(x_l, x_r, att, graph, self.negative_slope, n_dst)
        else:
            alpha = self.edge_updater(edge_index, x=(x_l, x_r), edge_attr=edge_attr)
            out = self.propagate(edge_index, x=(x_l, x_r), alpha=alpha)

        out = out.reshape(-1, H * C) if self.concat else out.mean(dim=1)
        if res is not None:
            out = out + res
        # a ReLU stack's request (BasicGNN, _act_request): bias + the model's activation in one pass
        fa = requested_activation(self)
        if fa is not None or (self.bias is not None and out.is_cuda):
            out = bias_act(out, self.bias, fa == 'relu')
        elif self.bias is not None:
            out = out + self.bias
        if low is not None and not torch.is_autocast_enabled():
            out = out.to(low)
        if not want_alpha:
            return out
        coo = edge_index.edge_index if isinstance(edge_index, EdgeIndex) else edge_index
        return out, (coo, alpha)

    def edge_update(self, x_j: Tensor, x_i: Tensor, edge_attr: Optional[Tensor], index: Tensor,
                    ptr: Optional[Tensor], dim_size: Optional[int]) -> Tensor:
        x = x_i + x_j
        if edge_attr is not None:
            e = edge_attr.view(-1, 1) if edge_attr.dim() == 1 else edge_attr
            assert self.lin_edge is not None
            x = x + self.lin_edge(e).view(-1, self.heads, self.out_channels)
        x = F.leaky_relu(x, self.negative_slope)
        att = self.att if self.att.dtype == x.dtype else self.att.to(x.dtype)
        alpha = (x * att).sum(dim=-1)
        if index.numel() > 0:
            alpha = softmax(alpha, index, ptr, dim_size)
        return F.dropout(alpha, p=self.dropout, training=self.training)

    def message(self, x_j: Tensor, alpha: Tensor) -> Tensor:
        return x_j * alpha.unsqueeze(-1)

    def __repr__(self) -> str:
        return (f'{type(self).__name__}({self.in_channels}, {self.out_channels}, '
                f'heads={self.heads})')
