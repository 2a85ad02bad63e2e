import math
import os
from typing import Optional, Tuple, Union

import torch
import torch.nn.functional as F
from torch import Tensor

from ... import _native
from ..._functions import (SegmentFunction, SpmmFunction, TransformerAttendFunction,
                           TransformerEdgeAttendFunction, TransformerEdgeScoreFunction,
                           TransformerScoreFunction, linear)
from ...edge_index import EdgeIndex, as_edge_index
from .._host import softmax
from ..dense.linear import Linear
from .message_passing import MessagePassing

# PYGAMD_FUSE_EDGE=1: layers with ``edge_dim`` start with ``fuse_edge = True`` (read at import)
FUSE_EDGE = os.environ.get('PYGAMD_FUSE_EDGE', '0') not in ('', '0')


class TransformerConv(MessagePassing):
    r"""Graph transformer operator with the constructor arguments, parameter names (``lin_key``,
    ``lin_query``, ``lin_value``, optional ``lin_edge``, ``lin_skip``, optional ``lin_beta``) and
    forward semantics of ``torch_geometric.nn.TransformerConv``
    (torch_geometric/nn/conv/transformer_conv.py:16-287):

    .. math:: \alpha_{ij} = \mathrm{softmax}_j \frac{(W_q x_i)^\top (W_k x_j + W_e e_{ij})}{\sqrt{C}},
              \qquad x_i' = W_s x_i + \big\Vert_h \sum_j \alpha^h_{ij} (W_v^h x_j + W_e e_{ij})

    (or the head mean; with ``beta`` the skip term and the aggregate are mixed by the gate
    ``sigmoid(w^\top [out, x_r, out - x_r])``).  The layer adds no self-loops.  Routes:

    * fused (float32 device tensors, no edge features, nothing between score and aggregation
      observable): key and value come from ONE projection of the sources over ``cat(W_k, W_v)``;
      ONE kernel per destination row keeps the query in registers, gathers each key and value row
      once and runs the score, an online softmax and the weighted sum
      (``TransformerAttendFunction``); the packed key | value gradient feeds one input-gradient
      product;
    * score mode (dropout on the coefficients in training, ``return_attention_weights``): the same
      kernel writes ``alpha [E, H]`` only, the multi-head weighted SpMM aggregates ``value``.  As
      in the reference the coefficients are returned as they are BEFORE dropout
      (transformer_conv.py:274-276), whenever the argument is a ``bool``, in the caller's edge
      order;
    * fused with edge features (``edge_dim`` layers with ``fuse_edge = True`` and a 2-D float
      device ``edge_attr [E, edge_dim]``, under the same other conditions, and
      ``_native.transformer_edge_supported(H, C, edge_dim)``): the edge term is linear, so it
      never exists per edge at width ``H * C``.  With ``W_e^h`` head ``h``'s block of
      ``lin_edge.weight``, ``b = scale * (W_e^h)^T q_i^h`` is a per-destination score bias and
      ``z_i^h = sum_k alpha a_k`` a per-destination sum of the RAW features; the same one-pass
      kernel reads ``De`` floats per slot and accumulates ``z`` beside the output
      (``TransformerEdgeAttendFunction``), and ``out = out_nodes + W_e z``.  The two products with
      ``W_e`` are plain einsums over nodes, so autograd carries their gradients.  In score mode
      the edge score node gives ``alpha``; after dropout the weighted SpMM aggregates ``value``
      and ``z`` is formed in tensor code (``w[k,h] * a_k`` as ``[E, H * edge_dim]``, reduced by
      the segment sum over the destination rows);
    * generic gather -> ``message`` -> scatter for ``edge_dim`` layers with ``fuse_edge = False``,
      ``fuse = False``, ``target_to_source`` and layouts the kernels do not serve (``H * C >
      512``, ``H > 64``, ``edge_dim`` beyond the edge registers) and for host tensors.

    ``fuse_edge`` is a per-layer attribute initialised from the environment switch
    ``PYGAMD_FUSE_EDGE``, which is read at import and defaults to ``0``: with default settings
    ``edge_dim`` layers take the generic route, which ``test_routing_to_the_generic_route`` in
    ``tests/test_gpu_transformer.py`` pins.  Flipping the default is a later change of its own,
    once the timings of ``profiles/transformer_conv_edge.md`` exist.

    Not offered: ``SparseTensor`` inputs, routing of the reference's own class through
    ``backend.install()``, a ``BasicGNN`` model of this layer.  The epilogue (head mean,
    ``lin_skip``, the ``lin_beta`` gate) is plain tensor code.
    """

    def __init__(self, in_channels: Union[int, Tuple[int, int]], out_channels: int,
                 heads: int = 1, concat: bool = True, beta: bool = False, dropout: float = 0.,
                 edge_dim: Optional[int] = None, bias: bool = True, root_weight: bool = True,
                 **kwargs):
        kwargs.setdefault('aggr', 'add')
        super().__init__(node_dim=0, **kwargs)
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.beta = beta and root_weight
        self.root_weight, self.concat, self.dropout = root_weight, concat, dropout
        self.edge_dim = edge_dim
        self.fuse_edge = FUSE_EDGE
        self._alpha = None
        in_src, in_dst = (in_channels, in_channels) if isinstance(in_channels, int) \
            else in_channels
        width = heads * out_channels
        self.lin_key = Linear(in_src, width, bias=bias)
        self.lin_query = Linear(in_dst, width, bias=bias)
        self.lin_value = Linear(in_src, width, bias=bias)
        if edge_dim is not None:
            self.lin_edge = Linear(edge_dim, width, bias=False)
        else:
            self.lin_edge = self.register_parameter('lin_edge', None)
        out_width = width if concat else out_channels
        self.lin_skip = Linear(in_dst, out_width, bias=bias)
        if self.beta:
            self.lin_beta = Linear(3 * out_width, 1, bias=False)
        else:
            self.lin_beta = self.register_parameter('lin_beta', None)
        self.fuse = True
        self.reset_parameters()

    def reset_parameters(self):
        super().reset_parameters()
        self.lin_key.reset_parameters()
        self.lin_query.reset_parameters()
        self.lin_value.reset_parameters()
        if self.edge_dim:
            self.lin_edge.reset_parameters()
        self.lin_skip.reset_parameters()
        if self.beta:
            self.lin_beta.reset_parameters()

    def forward(self, x: Union[Tensor, Tuple[Tensor, Tensor]], edge_index,
                edge_attr: Optional[Tensor] = None,
                return_attention_weights: Optional[bool] = None):
        H, C = self.heads, self.out_channels
        W = H * C
        if isinstance(x, Tensor):
            x = (x, x)
        x_src, x_dst = x[0], x[1]
        # the reference hands the coefficients back whenever the argument is a bool, True or False
        # (transformer_conv.py:254)
        want_alpha = isinstance(return_attention_weights, bool)
        native = (x_src.is_cuda and x_src.dtype in (torch.float32, torch.float16, torch.bfloat16)
                  and self.fuse and self.flow == 'source_to_target'
                  and _native.transformer_supported(H, C))
        edge = False
        if native and (edge_attr is not None or self.lin_edge is not None):
            edge = native = (
                self.fuse_edge and self.lin_edge is not None and isinstance(edge_attr, Tensor)
                and edge_attr.is_cuda and edge_attr.dim() == 2
                and edge_attr.size(1) == self.edge_dim and edge_attr.is_floating_point()
                and _native.transformer_edge_supported(H, C, self.edge_dim))
        scale = 1.0 / math.sqrt(C)
        alpha = None
        low = None
        if native:
            score_mode = want_alpha or (self.training and self.dropout > 0)
            query = self.lin_query(x_dst)
            if score_mode:
                key, value = self.lin_key(x_src), self.lin_value(x_src)
            else:
                # ONE projection for key and value; the parameters stay separate in the state dict
                kv = self._project_key_value(x_src)
            # the kernels compute in float32: half / bf16 projections are widened here and the
            # result handed back in their dtype outside autocast (as GATv2Conv does)
            if query.dtype in (torch.float16, torch.bfloat16):
                low = query.dtype
                query = query.float()
                if score_mode:
                    key, value = key.float(), value.float()
                else:
                    kv = kv.float()
            n_src, n_dst = x_src.size(0), x_dst.size(0)
            graph = as_edge_index(edge_index, n_src, n_dst)
            query = query.view(-1, H, C)
            if edge:
                out, alpha = self._attend_edge(query, key if score_mode else kv,
                                               value if score_mode else None, edge_attr, graph,
                                               scale, n_dst, score_mode, want_alpha)
            elif score_mode:
                # the coefficients are observable (dropout acts on them, or the caller asked):
                # score kernel -> dropout -> multi-head weighted SpMM over value
                alpha_slot = TransformerScoreFunction.apply(query, key.view(-1, H, C), graph,
                                                            scale, n_dst)
                weights = F.dropout(alpha_slot, p=self.dropout, training=self.training)
                out = SpmmFunction.apply(value.reshape(n_src, W), weights, graph, 'sum', 'slot')
                out = out.view(-1, H, C)
                if want_alpha:
                    # the PRE-dropout coefficients (self._alpha is set before F.dropout,
                    # transformer_conv.py:274-276), back in the caller's edge order
                    alpha = torch.empty_like(alpha_slot)
                    alpha[graph.by_dst().perm.long()] = alpha_slot
            else:
                out = TransformerAttendFunction.apply(query, kv.view(-1, 2, H, C), None, graph,
                                                      scale, n_dst)
        else:
            query = self.lin_query(x_dst).view(-1, H, C)
            key = self.lin_key(x_src).view(-1, H, C)
            value = self.lin_value(x_src).view(-1, H, C)
            out = self.propagate(edge_index, query=query, key=key, value=value,
                                 edge_attr=edge_attr)
            alpha, self._alpha = self._alpha, None

        out = out.reshape(-1, W) if self.concat else out.mean(dim=1)
        if low is not None:
            out = out.to(low) if not torch.is_autocast_enabled() else out
        if self.root_weight:
            x_r = self.lin_skip(x_dst)
            if x_r.dtype != out.dtype:
                x_r = x_r.to(out.dtype)
            if self.lin_beta is not None:
                gate = self.lin_beta(torch.cat([out, x_r, out - x_r], dim=-1)).sigmoid()
                out = gate * x_r + (1 - gate) * out
            else:
                out = out + x_r
        if not want_alpha:
            return out
        assert alpha is not None
        coo = edge_index.edge_index if isinstance(edge_index, EdgeIndex) else edge_index
        return out, (coo, alpha)

    def _attend_edge(self, query: Tensor, key: Tensor, value: Optional[Tensor], edge_attr: Tensor,
                     graph, scale: float, n_dst: int, score_mode: bool, want_alpha: bool):
        """The fused route with edge features: ``(out [n_dst, H, C], alpha | None)``.  ``value``
        None: ``key`` is the packed key | value projection."""
        H, C, De = self.heads, self.out_channels, self.edge_dim
        W = H * C
        ea = edge_attr.float()
        w_e = self.lin_edge.weight.float().view(H, C, De)
        bias = scale * torch.einsum('nhc,hcd->nhd', query, w_e)
        alpha = None
        if not score_mode:
            out, z = TransformerEdgeAttendFunction.apply(query, key.view(-1, 2, H, C), None, ea,
                                                         bias, graph, scale, n_dst)
        else:
            n_src = key.size(0)
            alpha_slot = TransformerEdgeScoreFunction.apply(query, key.view(-1, H, C), ea, bias,
                                                            graph, scale, n_dst)
            weights = F.dropout(alpha_slot, p=self.dropout, training=self.training)
            out = SpmmFunction.apply(value.reshape(n_src, W), weights, graph, 'sum', 'slot')
            out = out.view(-1, H, C)
            # z = sum over the row of w[k,h] * a_k, in tensor code: [E, H * De], then the segment
            # sum over the destination rows
            fwd = graph.by_dst()
            ea_slot = ea.index_select(0, fwd.perm.long())
            z = SegmentFunction.apply(
                (weights.unsqueeze(-1) * ea_slot.unsqueeze(1)).reshape(-1, H * De), fwd.ptr,
                'sum').view(-1, H, De)
            if want_alpha:
                alpha = torch.empty_like(alpha_slot)
                alpha[fwd.perm.long()] = alpha_slot
        return out + torch.einsum('nhd,hcd->nhc', z, w_e), alpha

    def _project_key_value(self, x_src: Tensor) -> Tensor:
        """``[lin_key(x) | lin_value(x)]`` as one ``[N_src, 2 * H * C]`` product."""
        weight = torch.cat([self.lin_key.weight, self.lin_value.weight], dim=0)
        bias = None
        if self.lin_key.bias is not None:
            bias = torch.cat([self.lin_key.bias, self.lin_value.bias], dim=0)
        return linear(x_src, weight, bias)

    def message(self, query_i: Tensor, key_j: Tensor, value_j: Tensor,
                edge_attr: Optional[Tensor], index: Tensor, ptr: Optional[Tensor],
                size_i: Optional[int]) -> Tensor:
        if self.lin_edge is not None:
            assert edge_attr is not None
            edge_attr = self.lin_edge(edge_attr).view(-1, self.heads, self.out_channels)
            key_j = key_j + edge_attr
        alpha = (query_i * key_j).sum(dim=-1) / math.sqrt(self.out_channels)
        if index.numel() > 0:
            alpha = softmax(alpha, index, ptr, size_i)
        self._alpha = alpha
        alpha = F.dropout(alpha, p=self.dropout, training=self.training)
        out = value_j
        if edge_attr is not None:
            out = out + edge_attr
        return out * alpha.view(-1, self.heads, 1)

    def __repr__(self) -> str:
        return (f'{type(self).__name__}({self.in_channels}, {self.out_channels}, '
                f'heads={self.heads})')
