import os
import weakref
from typing import Optional

import torch
import torch.nn.functional as F
from torch import Tensor
from torch.nn import Parameter, ReLU

from ... import _native
from ..._functions import RGATAggregateFunction, linear
from ..._onepass import RgatForms
from ...edge_index import EdgeIndex
from .. import _host
from ..dense.linear import Linear
from ..inits import glorot, ones, zeros
from .gmm_conv import device_floats, stock_flow
from .message_passing import _LOW, MessagePassing

# PYGAMD_FUSE_RGAT: whether an RGATConv starts with ``fuse = True`` (read at import).  The default
# is 1 because the fused training step was measured faster than the generic one at all four
# shapes of profiles/rgat_conv.md: 5.8 against 21.4 ms (R = 4, H = 4, C = 32), 6.6 against 24.9 ms
# (the same within-relation), 5.5 against 21.6 ms (R = 16, H = 1, C = 64) and 3.1 against 6.2 ms
# (R = 64, H = 2, C = 32 on a sparse batch-sized graph).
_DEFAULT_FUSE_RGAT = '1'
FUSE_RGAT = os.environ.get('PYGAMD_FUSE_RGAT', _DEFAULT_FUSE_RGAT).strip() not in ('', '0')

_MODS = ('additive', 'scaled', 'f-additive', 'f-scaled')


def _as(t: Tensor, like: Tensor) -> Tensor:
    """a parameter in the dtype of the data it meets: a half / bf16 layer whose inputs were widened
    computes with float32 copies of its parameters"""
    return t if t.dtype == like.dtype else t.to(like.dtype)


def _softmax(src: Tensor, index: Tensor, ptr: Optional[Tensor], n: Optional[int]) -> Tensor:
    """the softmax by index of the generic route: the package's primitive (float32 on the device,
    plain torch on the host) and, for a device tensor of another dtype (float64), the host
    formula, which is plain tensor code and runs where its tensors live"""
    if src.is_cuda and src.dtype != torch.float32:
        index = index.long()
        shape = (n, ) + src.shape[1:]
        where = index.view(-1, *[1] * (src.dim() - 1)).expand_as(src)
        top = src.new_full(shape, float('-inf')).scatter_reduce(0, where, src.detach(), 'amax',
                                                                include_self=True)
        num = (src - top.index_select(0, index)).exp()
        den = src.new_zeros(shape).index_add_(0, index, num) + 1e-16
        return num / den.index_select(0, index)
    return _host.softmax(src, index, ptr, n)


class RGATConv(MessagePassing):
    r"""The relational graph attention operator with the constructor arguments, defaults, errors,
    parameter names and shapes (``q, k, bias, lin_edge.weight, e, att, basis | weight, w, l1, b1,
    l2, b2``), ``__repr__`` and forward semantics of ``torch_geometric.nn.RGATConv``
    (torch_geometric/nn/conv/rgat_conv.py:16-534); state dicts load from and into the reference's.
    With ``W_r [in, H C]`` the weight of relation ``r`` (dense, ``att @ basis`` under ``num_bases``,
    block-diagonal under ``num_blocks``):

    .. math:: s_{e} = \mathrm{LeakyReLU}(x_i W_r q + x_j W_r k\ (+\ a_e W_e^\top e)), \quad
        x_i' = \sum_{e = (j, r, i)} \mathrm{softmax}(s)_e \cdot x_j W_r

    in the additive mode, the softmax over all edges into ``i`` (``'across-relation'``) or over
    those of relation ``r`` (``'within-relation'``); the multiplicative mode multiplies the terms
    and keeps ``dim`` scores per head.  ``return_attention_weights`` of either bool value returns
    ``(out, (edge_index, alpha))`` with ``alpha`` in the caller's edge order.  Routes:

    * fused (device tensors, float32 after widening, ``fuse`` true, ``flow='source_to_target'``,
      ``aggr`` add / sum, ``attention_mode='additive-self-attention'``, either
      ``attention_mechanism``, ``mod`` None, ``'scaled'`` or ``'f-scaled'``,
      dropout inactive (``p == 0`` or eval), with or without ``edge_dim``, ``H C <= 512``,
      ``H <= 64``): the weights of all relations and their products with ``q`` and ``k`` are folded
      on the parameters, ONE dense product gives the plane ``[P | QI | KJ] [N, R (H C + 2 H)]``
      (``P[:, r] = x W_r``, ``QI[:, r] = P[:, r] q``, ``KJ[:, r] = P[:, r] k``), the edge features
      one ``[E, H]`` score bias with the folded ``[edge_dim, H]`` weight, and all relations take
      ONE kernel forward and three backward (``RGATAggregateFunction``, csrc/rgat.hip) that gather
      one ``H C`` row and one scalar per edge and write one gradient plane: nothing of size ``E x
      H C`` or ``E x in`` is formed or saved.  ``'within-relation'`` adds one scalar launch over
      the ``(relation, destination)`` pairs in front of the forward (the pairs' normalisers).
      The head mean of ``concat=False``, the degree factor of ``mod`` (it depends on the
      destination only) and the bias are node-level torch code on the kernel's output.  The edges are sorted by relation, then by destination, once per
      ``(edge_index, edge_type)`` pair (cached on the layer by tensor identity and version);
    * generic (everything else: the multiplicative mode with ``dim >= 1``,
      ``mod`` ``'additive'`` / ``'f-additive'``, training dropout, host tensors, float64,
      ``fuse = False``, hooks, subclasses): this package's restatement through ``propagate``.  It
      gathers ``outi`` / ``outj`` from the plane ``P.view(N, R, H C)[idx, edge_type]`` — never a
      weight matrix per edge — and uses the softmax and scatter primitives; it runs on host
      tensors.

    The parameters follow the dtype of the data they meet, so a half / bf16 layer works on
    either route on the device.  An ``edge_type`` outside ``[0, num_relations)`` raises ``ValueError`` on both routes, and so
    does ``edge_type=None`` (``edge_index`` is a tensor or an ``EdgeIndex``, never a sparse
    matrix).  ``reset_parameters`` follows the reference's with one difference: the reference
    leaves ``l2`` as ``torch.empty`` (rgat_conv.py:310 discards the ``torch.full`` it builds);
    here ``l2`` IS filled with ``1 / out_channels``.  Half and bfloat16 device inputs are widened
    to float32 and the result handed back in their dtype outside autocast.  ``fuse`` is a
    per-layer attribute initialised from the environment switch ``PYGAMD_FUSE_RGAT`` (read at
    import)."""

    def __init__(self, in_channels: int, out_channels: int, num_relations: int,
                 num_bases: Optional[int] = None, num_blocks: Optional[int] = None,
                 mod: Optional[str] = None, attention_mechanism: str = 'across-relation',
                 attention_mode: str = 'additive-self-attention', heads: int = 1, dim: int = 1,
                 concat: bool = True, negative_slope: float = 0.2, dropout: float = 0.0,
                 edge_dim: Optional[int] = None, bias: bool = True, **kwargs):
        kwargs.setdefault('aggr', 'add')
        super().__init__(node_dim=0, **kwargs)
        self.heads = heads
        self.negative_slope = negative_slope
        self.dropout = dropout
        self.mod = mod
        self.activation = ReLU()
        self.concat = concat
        self.attention_mode = attention_mode
        self.attention_mechanism = attention_mechanism
        self.dim = dim
        self.edge_dim = edge_dim
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.num_relations = num_relations
        self.num_bases = num_bases
        self.num_blocks = num_blocks

        if attention_mechanism not in ('within-relation', 'across-relation'):
            raise ValueError('attention mechanism must either be '
                             '"within-relation" or "across-relation"')
        if attention_mode not in ('additive-self-attention', 'multiplicative-self-attention'):
            raise ValueError('attention mode must either be '
                             '"additive-self-attention" or '
                             '"multiplicative-self-attention"')
        if attention_mode == 'additive-self-attention' and dim > 1:
            raise ValueError('"additive-self-attention" mode cannot be '
                             'applied when value of d is greater than 1. '
                             'Use "multiplicative-self-attention" instead.')
        if dropout > 0.0 and mod in _MODS:
            raise ValueError('mod must be None with dropout value greater '
                             'than 0 in order to sample attention '
                             'coefficients stochastically')
        if num_bases is not None and num_blocks is not None:
            raise ValueError('Can not apply both basis-decomposition and '
                             'block-diagonal-decomposition at the same time.')

        W = heads * out_channels
        self.q = Parameter(torch.empty(W, heads * dim))
        self.k = Parameter(torch.empty(W, heads * dim))
        if bias and concat:
            self.bias = Parameter(torch.empty(heads * dim * out_channels))
        elif bias and not concat:
            self.bias = Parameter(torch.empty(dim * out_channels))
        else:
            self.register_parameter('bias', None)
        if edge_dim is not None:
            self.lin_edge = Linear(edge_dim, W, bias=False, weight_initializer='glorot')
            self.e = Parameter(torch.empty(W, heads * dim))
        else:
            self.lin_edge = None
            self.register_parameter('e', None)
        if num_bases is not None:
            self.att = Parameter(torch.empty(num_relations, num_bases))
            self.basis = Parameter(torch.empty(num_bases, in_channels, W))
        elif num_blocks is not None:
            assert in_channels % num_blocks == 0 and W % num_blocks == 0, (
                "both 'in_channels' and 'heads * out_channels' must be "
                "multiple of 'num_blocks' used")
            self.weight = Parameter(torch.empty(num_relations, num_blocks,
                                                in_channels // num_blocks, W // num_blocks))
        else:
            self.weight = Parameter(torch.empty(num_relations, in_channels, W))
        self.w = Parameter(torch.ones(out_channels))
        self.l1 = Parameter(torch.empty(1, out_channels))
        self.b1 = Parameter(torch.empty(1, out_channels))
        self.l2 = Parameter(torch.empty(out_channels, out_channels))
        self.b2 = Parameter(torch.empty(1, out_channels))
        self.fuse = FUSE_RGAT
        self.reset_parameters()

    def reset_parameters(self):
        super().reset_parameters()
        if self.num_bases is not None:
            glorot(self.basis)
            glorot(self.att)
        else:
            glorot(self.weight)
        glorot(self.q)
        glorot(self.k)
        zeros(self.bias)
        ones(self.l1)
        zeros(self.b1)
        with torch.no_grad():  # (the reference builds this tensor and drops it: see the docstring)
            self.l2.fill_(1 / self.out_channels)
        zeros(self.b2)
        if self.lin_edge is not None:
            self.lin_edge.reset_parameters()
            glorot(self.e)

    # -- shared pieces ----------------------------------------------------------------------------
    def _dense_weight(self) -> Tensor:
        """``[R, in, H C]``: the weights of all relations, torch code on the parameters"""
        R, W = self.num_relations, self.heads * self.out_channels
        if self.num_bases is not None:
            return (self.att @ self.basis.view(self.num_bases, -1)).view(R, self.in_channels, W)
        if self.num_blocks is not None:
            return torch.stack([torch.block_diag(*self.weight[r].unbind(0)) for r in range(R)])
        return self.weight

    def _degree_factor(self, deg: Tensor) -> Tensor:
        """``psi(deg) [n, C]`` of ``mod='scaled'`` (rgat_conv.py:461-466)"""
        d = self.activation(deg.view(-1, 1) @ _as(self.l1, deg) + _as(self.b1, deg))
        return d @ _as(self.l2, deg) + _as(self.b2, deg)

    def _check_types(self, edge_index, edge_type: Optional[Tensor]) -> Tensor:
        if edge_type is None:
            raise ValueError("'edge_type' is required: 'edge_index' is a tensor or an EdgeIndex "
                             "handle and carries no relations")
        E = (edge_index.edge_index if isinstance(edge_index, EdgeIndex) else edge_index).size(1)
        if edge_type.dim() != 1 or edge_type.numel() != E:
            raise ValueError(f"'edge_type' must hold one entry per edge (got "
                             f"{tuple(edge_type.shape)} for {E} edges)")
        return edge_type

    def _fusable(self, x) -> bool:
        if not stock_flow(self, RGATConv):
            return False
        return bool(self.fuse and self.flow == 'source_to_target' and self.aggr in ('add', 'sum')
                    and self.attention_mode == 'additive-self-attention'
                    and self.mod in (None, 'scaled', 'f-scaled')
                    and not (self.training and self.dropout > 0)
                    and device_floats(x) and x.size(1) == self.in_channels
                    and self.heads * self.out_channels <= 512 and self.heads <= 64)

    def forward(self, x: Tensor, edge_index, edge_type: Optional[Tensor] = None,
                edge_attr: Optional[Tensor] = None, size=None, return_attention_weights=None):
        edge_type = self._check_types(edge_index, edge_type)
        if edge_attr is not None:
            if edge_attr.dim() == 1:
                edge_attr = edge_attr.view(-1, 1)
            assert self.lin_edge is not None, (
                "Please set 'edge_dim = edge_attr.size(-1)' while calling the RGATConv layer")
        if self.num_blocks is not None and x.dtype == torch.long:
            raise ValueError('Block-diagonal decomposition not supported '
                             'for non-continuous input features.')
        ei = edge_index.edge_index if isinstance(edge_index, EdgeIndex) else edge_index
        fused = (self._fusable(x) and (edge_attr is None or device_floats(edge_attr))
                 and edge_type.is_cuda and ei.is_cuda)
        if fused:
            out, alpha = self._forward_fused(x, edge_index, edge_type, edge_attr, size)
        else:
            out, alpha = self._forward_generic(x, edge_index, edge_type, edge_attr, size)
        if isinstance(return_attention_weights, bool):
            return out, (edge_index, alpha)
        return out

    # -- fused ------------------------------------------------------------------------------------
    def _forms(self, ei: Tensor, edge_type: Tensor, n_src: int, n_dst: int) -> RgatForms:
        """The layer's sorted forms for this ``(edge_index, edge_type)`` pair, cached by tensor
        identity + in-place version: the sorts run once per graph, not per call."""
        hit = self.__dict__.get('_rgat_cache')
        if hit is not None:
            r_ei, r_et, v_ei, v_et, key, forms = hit
            if (r_ei() is ei and r_et() is edge_type and v_ei == ei._version
                    and v_et == edge_type._version and key == (n_src, n_dst)):
                return forms
        et = edge_type.to(torch.int64)
        if et.numel() > 0:
            lo, hi = _native.index_minmax(et)
            if lo < 0 or hi >= self.num_relations:
                raise ValueError(f"'edge_type' must lie in [0, {self.num_relations}) (got values "
                                 f"in [{lo}, {hi}])")
        forms = RgatForms.of_edges(ei[0].contiguous(), ei[1].contiguous(), et, n_src, n_dst,
                                   self.num_relations)
        self.__dict__['_rgat_cache'] = (weakref.ref(ei), weakref.ref(edge_type), ei._version,
                                        edge_type._version, (n_src, n_dst), forms)
        return forms

    def _forward_fused(self, x, edge_index, edge_type, edge_attr, size):
        H, C, R = self.heads, self.out_channels, self.num_relations
        W = H * C
        low = x.dtype if x.dtype in _LOW else None
        xf = x.float()
        N = xf.size(0)
        if isinstance(edge_index, EdgeIndex):
            n_src, n_dst = edge_index.num_src_nodes, edge_index.num_dst_nodes
            ei = edge_index.edge_index
        else:
            n_src, n_dst = (N, N) if size is None else (int(size[0]), int(size[1]))
            ei = edge_index
        if n_src > N or n_dst > N:
            raise ValueError(f"'x' has {N} rows, the graph needs ({n_src}, {n_dst})")
        forms = self._forms(ei, edge_type, n_src, n_dst)
        with torch.autocast('cuda', enabled=False):
            w = self._dense_weight().float()                              # [R, in, W]
            wq, wk = w @ self.q.float(), w @ self.k.float()               # [R, in, H]
            full = torch.cat([w.permute(1, 0, 2).reshape(-1, R * W),
                              wq.permute(1, 0, 2).reshape(-1, R * H),
                              wk.permute(1, 0, 2).reshape(-1, R * H)], dim=1)
            # ONE [N, R (W + 2H)] projection [P | QI | KJ] (the kernels read its blocks in place)
            plane = linear(xf, full.t().contiguous(), None)
            b = None
            if edge_attr is not None:
                fold = self.lin_edge.weight.float().t() @ self.e.float()  # [edge_dim, H]
                b = edge_attr.float() @ fold
            out, alpha = RGATAggregateFunction.apply(
                plane, None, None, b, forms, H, C, self.negative_slope,
                self.attention_mechanism == 'within-relation')
            out = out.view(-1, H, C)
            if self.mod == 'scaled':
                out = out * self._degree_factor(forms.deg).view(-1, 1, C)
            elif self.mod == 'f-scaled':
                out = out * forms.deg.view(-1, 1, 1)
            out = out.reshape(-1, W) if self.concat else out.mean(dim=1)
            if self.bias is not None:
                out = out + self.bias.float()
        if low is not None and not torch.is_autocast_enabled():
            out, alpha = out.to(low), alpha.to(low)
        return out, alpha

    # -- generic ----------------------------------------------------------------------------------
    def _forward_generic(self, x, edge_index, edge_type, edge_attr, size):
        low = x.dtype if (x.is_cuda and x.dtype in _LOW) else None
        if low is not None:
            x = x.float()
            edge_attr = None if edge_attr is None else edge_attr.float()
        R, W = self.num_relations, self.heads * self.out_channels
        if edge_type.numel() > 0:
            lo, hi = int(edge_type.min()), int(edge_type.max())
            if lo < 0 or hi >= R:
                raise ValueError(f"'edge_type' must lie in [0, {R}) (got values in [{lo}, {hi}])")
        w = self._dense_weight().to(x.dtype)
        plane = (x @ w.permute(1, 0, 2).reshape(-1, R * W)).view(-1, R, W)
        if size is None and not isinstance(edge_index, EdgeIndex):
            size = (x.size(0), x.size(0))
        out = self.propagate(edge_index, size=size, plane=plane, edge_type=edge_type,
                             edge_attr=edge_attr)
        alpha, self._alpha = self._alpha, None
        if low is not None and not torch.is_autocast_enabled():
            out, alpha = out.to(low), alpha.to(low)
        return out, alpha

    def message(self, plane: Tensor, edge_type: Tensor, edge_attr: Optional[Tensor],
                edge_index_i: Tensor, edge_index_j: Tensor, index: Tensor,
                ptr: Optional[Tensor], size_i: Optional[int]) -> Tensor:
        H, C, D = self.heads, self.out_channels, self.dim
        et = edge_type.long()
        outi = plane[edge_index_i.long(), et]                             # [E, H C]
        outj = plane[edge_index_j.long(), et]
        qi, kj = outi @ _as(self.q, plane), outj @ _as(self.k, plane)
        additive = self.attention_mode == 'additive-self-attention'
        if edge_attr is not None:
            edge = edge_attr @ _as(self.lin_edge.weight, plane).t()
            alpha_edge = edge.view(-1, H * C) @ _as(self.e, plane)
            alpha = qi + kj + alpha_edge if additive else (qi * kj) * alpha_edge
        else:
            alpha = qi + kj if additive else qi * kj
        if additive:
            alpha = F.leaky_relu(alpha, self.negative_slope)
        if self.attention_mechanism == 'within-relation':
            parts = torch.zeros_like(alpha)
            for r in range(self.num_relations):
                mask = et == r
                if bool(mask.any()):
                    parts = parts.index_put((mask.nonzero().view(-1), ),
                                            _softmax(alpha[mask], index[mask], None, size_i))
            alpha = parts
        else:
            alpha = _softmax(alpha, index, ptr, size_i)
        self._alpha = alpha

        def heads_of(t):  # [E, H, C] (additive) or [E, H, 1, C]
            return t.view(-1, H, C) if additive else t.view(-1, H, 1, C)

        def scores_of(a):  # [E, H, 1] or [E, H, dim, 1]
            return a.view(-1, H, 1) if additive else a.view(-1, H, D, 1)

        def degree():
            n = size_i if size_i is not None else (int(index.max()) + 1 if index.numel() else 0)
            return torch.bincount(index.long(), minlength=n).to(alpha.dtype)[index.long()]

        if self.mod == 'additive':
            h = _as(self.w, plane) * (heads_of(outj) * scores_of(torch.ones_like(alpha)))
            return heads_of(outj) * scores_of(alpha) + h
        if self.mod == 'scaled':
            factor = self._degree_factor(degree())
            return (heads_of(outj) * scores_of(alpha)) * (
                factor.view(-1, 1, C) if additive else factor.view(-1, 1, 1, C))
        if self.mod == 'f-additive':
            alpha = torch.where(alpha > 0, alpha + 1, alpha)
        elif self.mod == 'f-scaled':
            alpha = alpha * degree().unsqueeze(-1)
        elif self.training and self.dropout > 0:
            alpha = F.dropout(alpha, p=self.dropout, training=True)
        return scores_of(alpha) * heads_of(outj)

    def aggregate(self, inputs: Tensor, index: Tensor, ptr: Optional[Tensor] = None,
                  dim_size: Optional[int] = None) -> Tensor:
        if inputs.is_cuda and inputs.dtype != torch.float32:   # (float64: plain tensor code)
            return _host.aggregate(self.aggr_module, inputs, index, dim_size)
        return super().aggregate(inputs, index, ptr=ptr, dim_size=dim_size)

    def update(self, aggr_out: Tensor) -> Tensor:
        H, C, D = self.heads, self.out_channels, self.dim
        additive = self.attention_mode == 'additive-self-attention'
        if self.concat:
            aggr_out = aggr_out.reshape(-1, H * C if additive else H * D * C)
        else:
            aggr_out = aggr_out.mean(dim=1)
            if not additive:
                aggr_out = aggr_out.reshape(-1, D * C)
        if self.bias is not None:
            aggr_out = aggr_out + _as(self.bias, aggr_out)
        return aggr_out

    def __repr__(self) -> str:
        return '{}({}, {}, heads={})'.format(self.__class__.__name__, self.in_channels,
                                             self.out_channels, self.heads)
