import math
from types import SimpleNamespace
from typing import Dict, List, Optional, Tuple, Union

import torch
import torch.nn.functional as F
from torch import Tensor
from torch.nn import Parameter

from ... import _hgt
from ..._functions import HgtRelationPlan, HGTRelationFunction, TransformerAttendFunction
from .._host import softmax
from ..dense.linear import HeteroDictLinear, HeteroLinear, hetero_linear_forward
from .message_passing import MessagePassing


class HGTConv(MessagePassing):
    r"""The Heterogeneous Graph Transformer operator with the constructor arguments, parameter
    names (``kqv_lin.lins.<t>``, ``out_lin.lins.<t>``, ``k_rel.weight`` / ``v_rel.weight``
    ``[H * T, D, D]``, ``skip.<t>``, ``p_rel.<src>__<rel>__<dst>``) and forward semantics of
    ``torch_geometric.nn.HGTConv`` (torch_geometric/nn/conv/hgt_conv.py:17-236): per node type one
    key | query | value projection; per edge type and head a ``D x D`` relation matrix on the keys
    and on the values of its source nodes; a dot-product attention whose softmax runs over ALL
    incoming edges of a destination, across edge types, with the score of edge type ``e`` scaled
    by ``p_rel[e][h] / sqrt(D)``; GELU, ``out_lin`` and — where the input width equals
    ``out_channels`` — the ``sigmoid(skip)`` mix with the input.  The result holds the node types
    of ``x_dict`` that are a destination in the metadata.  Routes:

    * fused (float32 device tensors, ``fuse``, ``source_to_target``, nobody observing
      ``propagate`` / ``message``, ``H * D <= 512``, ``H <= 64``, ``D <= 128``): ``kqv_lin``; ONE
      relation-transform launch for every edge type (``HGTRelationFunction``: rows read in place
      from the projection, weights in the parameters' layout, ``p_rel`` folded into the key
      matrices); ONE attention launch over the cached stacked bipartite handle
      (``TransformerAttendFunction``); the epilogue in plain tensor code.  Nothing of size
      ``E x F`` exists, forward or backward;
    * generic (everything else, host tensors included): the reference's formulation over this
      package's ``HeteroLinear``, ``softmax`` and ``propagate`` (half / bf16 device rows are
      widened to float32 for it; host rows take a ``bmm`` over the gathered relation matrices).

    Not offered: lazy ``-1`` widths, ``SparseTensor`` inputs, ``to_hetero``, routing of the
    reference's own class through ``backend.install()``.
    """

    def __init__(self, in_channels: Union[int, Dict[str, int]], out_channels: int,
                 metadata: Tuple[List[str], List[Tuple[str, str, str]]], heads: int = 1,
                 **kwargs):
        super().__init__(aggr='add', node_dim=0, **kwargs)
        if out_channels % heads != 0:
            raise ValueError(f"'out_channels' (got {out_channels}) must be "
                             f"divisible by the number of heads (got {heads})")
        if not isinstance(in_channels, dict):
            in_channels = {node_type: in_channels for node_type in metadata[0]}
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.heads = heads
        self.node_types = list(metadata[0])
        self.edge_types = [tuple(et) for et in metadata[1]]
        self.edge_types_map = {et: i for i, et in enumerate(self.edge_types)}
        self.dst_node_types = {et[-1] for et in self.edge_types}
        # (HeteroDictLinear refuses lazy -1 widths)
        self.kqv_lin = HeteroDictLinear(self.in_channels, self.out_channels * 3)
        self.out_lin = HeteroDictLinear(self.out_channels, self.out_channels,
                                        types=self.node_types)
        dim = out_channels // heads
        num_types = heads * len(self.edge_types)
        self.k_rel = HeteroLinear(dim, dim, num_types, bias=False, is_sorted=True)
        self.v_rel = HeteroLinear(dim, dim, num_types, bias=False, is_sorted=True)
        # (filled one by one: the entries keep the metadata's order, as the reference's do)
        self.skip = torch.nn.ParameterDict()
        for node_type in self.node_types:
            self.skip[node_type] = Parameter(torch.empty(1))
        self.p_rel = torch.nn.ParameterDict()
        for et in self.edge_types:
            self.p_rel['__'.join(et)] = Parameter(torch.empty(1, heads))
        self.fuse = True
        self.reset_parameters()

    def reset_parameters(self):
        super().reset_parameters()
        self.kqv_lin.reset_parameters()
        self.out_lin.reset_parameters()
        self.k_rel.reset_parameters()
        self.v_rel.reset_parameters()
        for p in list(self.skip.values()) + list(self.p_rel.values()):
            torch.nn.init.ones_(p)

    # -- the call ---------------------------------------------------------------------------------
    def _call_edge_types(self, kqv_dict, edge_index_dict) -> List[Tuple[str, str, str]]:
        """The edge types of the call in metadata order (the order of the stacked source rows and
        of the sums of the backward); edge types absent from ``edge_index_dict`` are skipped."""
        ets = []
        for et in edge_index_dict:
            et = tuple(et)
            if et not in self.edge_types_map:
                raise KeyError(f'edge type {et} is not part of the metadata of this layer')
            if et[0] not in kqv_dict or et[-1] not in kqv_dict:
                raise KeyError(f"edge type {et} needs the features of '{et[0]}' and '{et[-1]}'")
            ets.append(et)
        return sorted(ets, key=self.edge_types_map.__getitem__)

    def forward(self, x_dict: Dict[str, Tensor],
                edge_index_dict: Dict[Tuple[str, str, str], Tensor]) -> Dict[str, Tensor]:
        W, H = self.out_channels, self.heads
        D = W // H
        kqv_dict = self.kqv_lin(x_dict)
        ets = self._call_edge_types(kqv_dict, edge_index_dict)
        eis = {et: edge_index_dict[et] for et in ets}
        st = _hgt.Stacking({t: v.size(0) for t, v in kqv_dict.items()}, ets)
        first = next(iter(kqv_dict.values()))
        low = None
        if first.is_cuda and _hgt.eligible(self, x_dict, ets, eis):
            out = self._attend_fused(kqv_dict, st, eis)
        else:
            if first.is_cuda and first.dtype in (torch.float16, torch.bfloat16):
                low = first.dtype
                kqv_dict = {t: v.float() for t, v in kqv_dict.items()}
            out = self._attend_generic(kqv_dict, st, eis)
            if low is not None and not torch.is_autocast_enabled():
                out = out.to(low)
        out = out.reshape(-1, W)
        # the node types of x_dict that are a destination in the metadata, with or without edges
        out_dict = {t: out[st.dst_off[t]:st.dst_off[t] + st.sizes[t]]
                    for t in st.node_types if t in self.dst_node_types}
        a_dict = self.out_lin({t: F.gelu(v) for t, v in out_dict.items()})
        for t in out_dict:
            o = a_dict[t]
            if o.size(-1) == x_dict[t].size(-1):
                alpha = self.skip[t].sigmoid()
                o = alpha * o + (1 - alpha) * x_dict[t]
            out_dict[t] = o
        return out_dict

    def _relation_scale(self) -> Tensor:
        """``p_rel`` as the ``[H * T, 1, 1]`` factor of the key matrices: row ``h * T + e``."""
        p = torch.cat([self.p_rel['__'.join(et)] for et in self.edge_types], dim=0)   # [T, H]
        return p.t().reshape(-1, 1, 1)

    def _query(self, kqv_dict) -> Tensor:
        W = self.out_channels
        qs = [v[:, W:2 * W] for v in kqv_dict.values()]
        return (qs[0] if len(qs) == 1 else torch.cat(qs, dim=0)).reshape(-1, self.heads,
                                                                        W // self.heads)

    def _attend_fused(self, kqv_dict, st: _hgt.Stacking, eis) -> Tensor:
        H, D = self.heads, self.out_channels // self.heads
        ets = st.edge_types
        q = self._query(kqv_dict)
        if not ets:   # no edge type in the call: every destination aggregates nothing
            return q * 0.0
        graph = _hgt.stacked_graph(st, [eis[et] for et in ets])
        src_types = list(dict.fromkeys(et[0] for et in ets))
        plan = HgtRelationPlan(H, [src_types.index(et[0]) for et in ets],
                               [self.edge_types_map[et] for et in ets])
        # the score's per-relation prior scales the key matrices: autograd carries p_rel's
        # gradient through the product
        wk = self.k_rel.weight * self._relation_scale()
        kv = HGTRelationFunction.apply(plan, wk, self.v_rel.weight,
                                       *[kqv_dict[t] for t in src_types])
        return TransformerAttendFunction.apply(q, kv.view(-1, 2, H, D), None, graph,
                                               1.0 / math.sqrt(D), st.num_dst)

    def _source_features(self, kqv_dict, st: _hgt.Stacking, relation):
        """hgt_conv.py:118-154: the stacked, head-major rows and their type vector through
        ``relation(k_rows, v_rows, type_vec)``; back as ``[S, H, D]`` each."""
        W, H = self.out_channels, self.heads
        D, T = W // H, len(self.edge_types)
        first = next(iter(kqv_dict.values()))
        ks = [kqv_dict[et[0]][:, :W].reshape(-1, H, D) for et in st.edge_types]
        vs = [kqv_dict[et[0]][:, 2 * W:].reshape(-1, H, D) for et in st.edge_types]
        if not ks:
            empty = first.new_zeros(0, H, D)
            return empty, empty
        heads = torch.arange(H, dtype=torch.long, device=first.device).view(-1, 1) * T
        type_vec = torch.cat([(heads + self.edge_types_map[et]).repeat(1, st.sizes[et[0]])
                              for et in st.edge_types], dim=1).flatten()
        k_rows = torch.cat(ks, dim=0).transpose(0, 1).reshape(-1, D)
        v_rows = torch.cat(vs, dim=0).transpose(0, 1).reshape(-1, D)
        k, v = relation(k_rows, v_rows, type_vec)
        return k.view(H, -1, D).transpose(0, 1), v.view(H, -1, D).transpose(0, 1)

    def _stacked_edges(self, st: _hgt.Stacking, eis, device):
        """``construct_bipartite_edge_index`` (utils/hetero.py:82-151): the stacked edge list and
        ``p_rel`` of every edge ``[E, H]``."""
        parts, priors = [], []
        for k, et in enumerate(st.edge_types):
            ei = eis[et]
            ei = (ei.edge_index if hasattr(ei, 'edge_index') else ei).long()
            shift = torch.tensor([[st.src_off[k]], [st.dst_off[et[-1]]]], device=ei.device)
            parts.append(ei + shift)
            priors.append(self.p_rel['__'.join(et)].expand(ei.size(1), -1))
        if not parts:
            return (torch.zeros(2, 0, dtype=torch.long, device=device),
                    torch.zeros(0, self.heads, device=device))
        return torch.cat(parts, dim=1), torch.cat(priors, dim=0)

    def _attend_generic(self, kqv_dict, st: _hgt.Stacking, eis) -> Tensor:
        q = self._query(kqv_dict)
        def relation(k_rows, v_rows, type_vec):
            if not k_rows.is_cuda:
                return (torch.bmm(k_rows.unsqueeze(1), self.k_rel.weight[type_vec]).squeeze(1),
                        torch.bmm(v_rows.unsqueeze(1), self.v_rel.weight[type_vec]).squeeze(1))
            if self.k_rel.weight.dtype == torch.float32:
                return self.k_rel(k_rows, type_vec), self.v_rel(v_rows, type_vec)
            # half / bf16 parameters: the grouped product computes in float32
            wide = [SimpleNamespace(weight=m.weight.float(), bias=None, num_types=m.num_types,
                                    is_sorted=True) for m in (self.k_rel, self.v_rel)]
            return (hetero_linear_forward(wide[0], k_rows, type_vec),
                    hetero_linear_forward(wide[1], v_rows, type_vec))

        k, v = self._source_features(kqv_dict, st, relation)
        edge_index, prior = self._stacked_edges(st, eis, q.device)
        # (the edge type names source and destination: row 0 of every edge_index is the source
        # type's id whatever the flow; under 'target_to_source' propagate wants the rows swapped)
        if self.flow == 'target_to_source':
            edge_index = edge_index.flip(0)
        size = (st.num_src, st.num_dst) if self.flow == 'source_to_target' \
            else (st.num_dst, st.num_src)
        return self.propagate(edge_index, k=k.contiguous(), q=q.contiguous(), v=v.contiguous(),
                              edge_attr=prior.to(q.dtype), size=size)

    def message(self, k_j: Tensor, q_i: Tensor, v_j: Tensor, edge_attr: Tensor, index: Tensor,
                ptr: Optional[Tensor], size_i: Optional[int]) -> Tensor:
        alpha = (q_i * k_j).sum(dim=-1) * edge_attr
        alpha = alpha / math.sqrt(q_i.size(-1))
        if index.numel() > 0:
            alpha = softmax(alpha, index, ptr, size_i)
        return v_j * alpha.view(-1, self.heads, 1)

    def __repr__(self) -> str:
        return f'{type(self).__name__}(-1, {self.out_channels}, heads={self.heads})'
