from typing import Dict, List, Optional, Tuple, Union

import torch
import torch.nn.functional as F
from torch import Tensor
from torch.nn import Parameter

from ... import _han
from ..._functions import HanAttendFunction
from .._host import softmax
from ..dense.linear import Linear
from ..inits import glorot
from .message_passing import _LOW, MessagePassing


def group(xs: List[Tensor], q: Tensor, k_lin: torch.nn.Module):
    """The semantic attention over the edge types that end in one node type (han_conv.py:15-31):
    ``(out, beta)``; ``(None, None)`` without an edge type, ``([0, F], None)`` without rows."""
    if len(xs) == 0:
        return None, None
    out = torch.stack(xs)
    if out.numel() == 0:
        return out.view(0, out.size(-1)), None
    score = (q * torch.tanh(k_lin(out)).mean(1)).sum(-1)
    attn = F.softmax(score, dim=0)
    return torch.sum(attn.view(len(xs), 1, -1) * out, dim=0), attn


class HANConv(MessagePassing):
    r"""The Heterogeneous Graph Attention Network operator with the constructor arguments, parameter
    names (``proj.<t>``, ``lin_src.<src>__<rel>__<dst>``, ``lin_dst.<src>__<rel>__<dst>``,
    ``k_lin``, ``q``) and forward semantics of ``torch_geometric.nn.HANConv``
    (torch_geometric/nn/conv/han_conv.py:34-183): one projection per node type; per edge type of
    the call GAT's additive attention over the incoming edges of that edge type,
    :math:`\alpha_{ij} = \mathrm{softmax}_j\,\mathrm{LeakyReLU}(a_s^\top x_j + a_d^\top x_i)`,
    dropout on :math:`\alpha` and :math:`z_e = \mathrm{ReLU}(\sum_j \alpha_{ij} x_j)`; per
    destination node type the semantic attention :math:`\beta = \mathrm{softmax}_e\,(q \cdot
    \mathrm{mean}_i \tanh(k\_lin(z_e)))` and :math:`\sum_e \beta_e z_e`.  A node type without an
    incoming edge type in the call maps to ``None``, one without rows to a ``[0, out_channels]``
    tensor with ``None`` weights; ``beta`` follows the order of ``edge_index_dict``.  Routes:

    * fused (float32 device tensors, ``fuse``, ``source_to_target``, nobody observing
      ``propagate`` / ``message`` / ``aggregate``, no dropout in training, ``H * D <= 512``,
      ``H <= 64``, at most 64 edge and node types): the projections stacked once per node type; the
      per-node logits in tensor code; ONE attention launch for every edge type over the cached
      stacked handle (``HanAttendFunction``, csrc/han.hip) and at most two in the backward; the
      semantic attention in plain tensor code on views of the kernel's output.  Nothing of size
      ``E x F`` exists, forward or backward;
    * generic (everything else, host tensors included): the reference's per-edge-type loop over
      this package's ``propagate`` (half / bf16 device rows are widened to float32 for it).

    ``fuse`` starts from ``PYGAMD_FUSE_HAN`` (read at import; default on).  Not offered: lazy ``-1``
    widths, ``SparseTensor`` inputs, ``to_hetero``, routing of the reference's own class through
    ``backend.install()``.
    """

    def __init__(self, in_channels: Union[int, Dict[str, int]], out_channels: int,
                 metadata: Tuple[List[str], List[Tuple[str, str, str]]], heads: int = 1,
                 negative_slope: float = 0.2, dropout: float = 0.0, **kwargs):
        super().__init__(aggr='add', node_dim=0, **kwargs)
        if out_channels % heads != 0:
            raise ValueError(f"'out_channels' (got {out_channels}) must be "
                             f"divisible by the number of heads (got {heads})")
        if not isinstance(in_channels, dict):
            in_channels = {node_type: in_channels for node_type in metadata[0]}
        self.heads = heads
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.negative_slope = negative_slope
        self.metadata = metadata
        self.dropout = dropout
        self.k_lin = Linear(out_channels, out_channels)
        self.q = Parameter(torch.empty(1, out_channels))
        self.proj = torch.nn.ModuleDict()
        for node_type, width in self.in_channels.items():   # (Linear refuses lazy -1 widths)
            self.proj[node_type] = Linear(width, out_channels)
        self.lin_src = torch.nn.ParameterDict()
        self.lin_dst = torch.nn.ParameterDict()
        dim = out_channels // heads
        for edge_type in metadata[1]:
            key = '__'.join(edge_type)
            self.lin_src[key] = Parameter(torch.empty(1, heads, dim))
            self.lin_dst[key] = Parameter(torch.empty(1, heads, dim))
        self.fuse = _han.FUSE_DEFAULT
        self.reset_parameters()

    def reset_parameters(self):
        super().reset_parameters()
        for lin in self.proj.values():
            lin.reset_parameters()
        for p in list(self.lin_src.values()) + list(self.lin_dst.values()):
            glorot(p)
        self.k_lin.reset_parameters()
        glorot(self.q)

    # -- the call ---------------------------------------------------------------------------------
    def _call_edge_types(self, x_node_dict, edge_index_dict) -> List[Tuple[str, str, str]]:
        """The edge types of the call in the order of ``edge_index_dict`` (the order of ``beta``)"""
        ets = []
        for et in edge_index_dict:
            et = tuple(et)
            if '__'.join(et) not in self.lin_src:
                raise KeyError(f'edge type {et} is not part of the metadata of this layer')
            if et[0] not in x_node_dict or et[-1] not in x_node_dict:
                raise KeyError(f"edge type {et} needs the features of '{et[0]}' and '{et[-1]}'")
            ets.append(et)
        return ets

    def forward(self, x_dict: Dict[str, Tensor],
                edge_index_dict: Dict[Tuple[str, str, str], Tensor],
                return_semantic_attention_weights: bool = False):
        x_node_dict = {t: self.proj[t](x) for t, x in x_dict.items()}
        ets = self._call_edge_types(x_node_dict, edge_index_dict)
        eis = {et: edge_index_dict[et] for et in ets}
        first = next(iter(x_node_dict.values()), None)
        if first is not None and first.is_cuda and _han.eligible(self, x_node_dict, ets, eis):
            out_dict, attn_dict = self._forward_fused(x_node_dict, ets, eis)
        else:
            out_dict, attn_dict = self._forward_generic(x_node_dict, ets, eis)
        if return_semantic_attention_weights:
            return out_dict, attn_dict
        return out_dict

    def _forward_fused(self, x_node_dict, ets, eis):
        H, D = self.heads, self.out_channels // self.heads
        st = _han.Stacking({t: v.size(0) for t, v in x_node_dict.items()}, ets)
        xs = list(x_node_dict.values())
        x_all = xs[0] if len(xs) == 1 else torch.cat(xs, dim=0)
        heads = {t: v.view(-1, H, D) for t, v in x_node_dict.items()}
        keys = ['__'.join(et) for et in ets]
        # the per-node logits, stacked like the graph; autograd carries their gradients
        a_src = [(heads[et[0]] * self.lin_src[k]).sum(dim=-1) for et, k in zip(ets, keys)]
        a_dst = [(heads[et[-1]] * self.lin_dst[k]).sum(dim=-1) for et, k in zip(ets, keys)]
        a_src = a_src[0] if len(ets) == 1 else torch.cat(a_src, dim=0)
        a_dst = a_dst[0] if len(ets) == 1 else torch.cat(a_dst, dim=0)
        graph = _han.stacked_graph(st, [eis[et] for et in ets])
        z, _ = HanAttendFunction.apply(x_all.view(-1, H, D), a_src, a_dst, graph, st.types,
                                       self.negative_slope, True)
        # semantic attention: k_lin once over every (edge type, destination) row, one mean per
        # edge-type block, a softmax per destination type over views of z
        blocks = [z[st.row_begin[e]:st.row_begin[e + 1]] for e in range(len(ets))]
        live = [e for e in range(len(ets)) if blocks[e].size(0) > 0]
        score = {}
        if live:
            k = torch.tanh(self.k_lin(z))
            means = torch.stack([k[st.row_begin[e]:st.row_begin[e + 1]].mean(dim=0)
                                 for e in live])
            score = dict(zip(live, (self.q * means).sum(dim=-1).unbind(0)))
        out_dict, attn_dict = {}, {}
        for t in x_node_dict:
            mine = [e for e, et in enumerate(ets) if et[-1] == t]
            if not mine:
                out_dict[t] = attn_dict[t] = None
            elif mine[0] not in score:   # a destination type without rows
                out_dict[t], attn_dict[t] = blocks[mine[0]], None
            else:
                beta = F.softmax(torch.stack([score[e] for e in mine]), dim=0)
                out = blocks[mine[0]] * beta[0]
                for i, e in enumerate(mine[1:], start=1):
                    out = out + blocks[e] * beta[i]
                out_dict[t], attn_dict[t] = out, beta
        return out_dict, attn_dict

    def _forward_generic(self, x_node_dict, ets, eis):
        H, D = self.heads, self.out_channels // self.heads
        low = None
        first = next(iter(x_node_dict.values()), None)
        if first is not None and first.is_cuda and first.dtype in _LOW:
            low = first.dtype
        heads = {t: (v.float() if low is not None else v).view(-1, H, D)
                 for t, v in x_node_dict.items()}
        out_lists = {t: [] for t in x_node_dict}
        for et in ets:
            key = '__'.join(et)
            x_src, x_dst = heads[et[0]], heads[et[-1]]
            alpha_src = (x_src * self.lin_src[key]).sum(dim=-1)
            alpha_dst = (x_dst * self.lin_dst[key]).sum(dim=-1)
            out = self.propagate(eis[et], x=(x_src, x_dst), alpha=(alpha_src, alpha_dst))
            out = F.relu(out)
            if low is not None and not torch.is_autocast_enabled():
                out = out.to(low)
            out_lists[et[-1]].append(out)
        out_dict, attn_dict = {}, {}
        for t, outs in out_lists.items():
            out_dict[t], attn_dict[t] = group(outs, self.q, self.k_lin)
        return out_dict, attn_dict

    def message(self, x_j: Tensor, alpha_i: Tensor, alpha_j: Tensor, index: Tensor,
                ptr: Optional[Tensor], size_i: Optional[int]) -> Tensor:
        alpha = alpha_j + alpha_i
        alpha = F.leaky_relu(alpha, self.negative_slope)
        if index.numel() > 0:
            alpha = softmax(alpha, index, ptr, size_i)
        alpha = F.dropout(alpha, p=self.dropout, training=self.training)
        out = x_j * alpha.view(-1, self.heads, 1)
        return out.view(-1, self.out_channels)

    def __repr__(self) -> str:
        return f'{type(self).__name__}({self.out_channels}, heads={self.heads})'
